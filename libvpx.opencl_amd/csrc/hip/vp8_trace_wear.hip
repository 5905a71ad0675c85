// Trace wear (vp8hip_frames_wear_async and vp8hip_trace_wear_async, vp8hip_trace.hip; include/vp8hip.h has the definitions).  The
// WEAR of a frame says, for every pixel of the display-size luma grid, what happened on the way its trace took to the anchor
// picture: one dword per pixel, four saturating byte counters -- HOPS (byte 0), INTRA (1), EDGE (2), CODED (3).  An inter frame's
// wear is one hop: the pixel takes the dword the reference's wear holds where its trace went, and every byte goes up by the hop's
// 0 / 1 increment.  Wear entries live in a pool of a trace pool's geometry in the caller's device memory.
//
// vp8_wear_kernel, shaped as vp8_trace_kernel (vp8_trace.hip): a workgroup takes a group of R macroblock rows, stages the rows'
// vectors (16-byte loads) and ONE dword per macroblock -- ref_frame in the low byte and above it the mask of the luma blocks whose
// CODED increment is 1, made by a lane per macroblock from the record's first dword, eobs[0..15] and eobs[24] (one 64-byte half
// line) -- 68 bytes of LDS a macroblock, as the trace.  Then a lane makes four neighbouring pixels of one 4x4 block's row: one
// vector, one reference, one increment dword (byte 2, EDGE, differs among the four only where the group straddles the picture's
// edge), one 16-byte load of the reference's wear where the clamp does not bite.  A key frame writes zeros and reads nothing.
// Stores as in vp8_side.hip.  Job, references and the key-frame bit travel in the kernel arguments: the trace's TraceLaunch.
//
// vp8_wear_*_kernel.  A pool entry as a tensor [planes][gh][gw]: output (y, x) takes wear pixel (sy, sx) by the centre map, read
// through trace_read4 -- the pool has a trace pool's geometry --, and each plane asked for holds its counter's byte, converted as
// the side tensors are.
// Integer and conversion arithmetic only; wear values are data and never become addresses.
#include "vp8_trace_read.hip.h"
#include "vp8hip.h"

// P's four byte counters plus inc's (0 or 1 each), saturating at 255: `full` has a 1 in every byte of P that is 255 (the low seven
// bits all set carries into bit 7, which P has set too), and without those increments no byte carries into its neighbour
__device__ __forceinline__ unsigned wear_add(unsigned P, unsigned inc)
{
    const unsigned full = (((P & 0x7f7f7f7fu) + 0x01010101u) & P & 0x80808080u) >> 7;
    return P + (inc & ~full);
}

// grid: x = the groups of macroblock rows of a frame, y = the jobs of the launch.  slot_base: IR slot 0, slot_bytes apart, records
// at o_mbx and vectors at o_mvs inside; pool: entry 0, pool_stride apart.
extern "C" __global__ void __launch_bounds__(256)
vp8_wear_kernel(const char *__restrict__ slot_base, size_t slot_bytes, size_t o_mbx, size_t o_mvs, uint8_t *pool, size_t pool_stride, TraceLaunch L)
{
    extern __shared__ __attribute__((aligned(16))) unsigned wear_lds[];
    const TraceJob J = L.j[blockIdx.y];
    const int dw = L.dw, dh = L.dh, cols = L.mb_cols;
    const int m0 = (int)blockIdx.x * L.R, m1 = min(m0 + L.R, L.mb_rows);
    const int y0 = 16 * m0, y1 = min(16 * m1, dh);
    const bool key = J.key != 0;
    const unsigned *lrec = wear_lds + (size_t)L.R * cols * 16, *lmvs = wear_lds;          // vectors first: 16-byte pieces
    if (!key) {
        const char *slot = slot_base + slot_bytes * (size_t)J.slot;
        const GLOBAL_AS unsigned *grec = (const GLOBAL_AS unsigned *)(slot + o_mbx) + (size_t)m0 * cols * 32;
        const GLOBAL_AS u32x4_t *gmvs = (const GLOBAL_AS u32x4_t *)(slot + o_mvs) + (size_t)m0 * cols * 4;
        const int nmb = (m1 - m0) * cols;
#pragma unroll 1
        for (int t = threadIdx.x; t < nmb; t += 256) {
            // vp8ir_mb: y_mode, uv_mode, ref_frame, flags in dword 0; eobs[0..15] in dwords 2..5; eobs[24] the low byte of dword 8
            const GLOBAL_AS unsigned *rec = grec + t * 32;
            const unsigned d0 = rec[0], y2 = rec[8] & 255u;
            const u32x4_t eobs = load4_dword_aligned(rec + 2);
            const unsigned y_mode = d0 & 255u;
            const bool has_y2 = y_mode != VP8IR_B_PRED && y_mode != VP8IR_SPLITMV;
            // vp8ir_block_kind(m, k) != 0: eobs[k] > 1 beside a Y2 block, eobs[k] > 0 without; vp8ir_block_kind(m, 24) != 0: all sixteen
            const unsigned least = has_y2 ? 1u : 0u;
            unsigned mask = 0;
#pragma unroll
            for (int k = 0; k < 16; k++) mask |= (((eobs[k >> 2] >> (8 * (k & 3))) & 255u) > least ? 1u : 0u) << k;
            if (has_y2 && y2) mask = 0xffffu;
            if ((d0 >> 24) & VP8IR_MB_SKIP) mask = 0;
            wear_lds[(size_t)L.R * cols * 16 + t] = ((d0 >> 16) & 255u) | mask << 8;
        }
#pragma unroll 1
        for (int t = threadIdx.x; t < nmb * 4; t += 256) ((u32x4_t *)wear_lds)[t] = gmvs[t];
        __syncthreads();
    }

    uint8_t *D = pool + pool_stride * (size_t)J.dst;
    const int nrows = y1 - y0;
#pragma unroll 1
    for (TensorWalk t((dw + 3) >> 2); t.row < nrows; t.next()) {
        const int y = y0 + t.row, x = t.col << 2;
        unsigned e[4] = {0, 0, 0, 0};
        if (!key) {
            const int mb = ((y >> 4) - m0) * cols + (x >> 4);
            const unsigned rec = lrec[mb], ref = rec & 255u;
            // an intra macroblock is held in place through the last frame
            const int pi = ref <= VP8IR_LAST_FRAME ? J.ref[0] : ref == VP8IR_GOLDEN_FRAME ? J.ref[1] : ref == VP8IR_ALTREF_FRAME ? J.ref[2] : -1;
            if (pi >= 0) {
                const int k = ((y >> 2) & 3) * 4 + ((x >> 2) & 3);
                const unsigned v = ref == VP8IR_INTRA_FRAME ? 0u : lmvs[mb * 16 + k];
                const int dx = (((int)v >> 16) + 4) >> 3, dy = ((int)(short)(v & 0xffffu) + 4) >> 3;       // col in the high half
                const int uy = y + dy, sy = min(max(uy, 0), dh - 1), sx = x + dx;
                // HOPS, INTRA, the row's share of EDGE, CODED
                const unsigned inc = 1u | (ref == VP8IR_INTRA_FRAME ? 1u << 8 : 0u) | (sy != uy ? 1u << 16 : 0u) | ((rec >> (8 + k)) & 1u) << 24;
                const GLOBAL_AS unsigned *row = (const GLOBAL_AS unsigned *)(pool + pool_stride * (size_t)pi) + (size_t)sy * dw;
                if (sx >= 0 && sx + 3 < dw) {
                    const u32x4_t g = load4_dword_aligned(row + sx);
                    e[0] = wear_add(g.x, inc); e[1] = wear_add(g.y, inc); e[2] = wear_add(g.z, inc); e[3] = wear_add(g.w, inc);
                } else {
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const int cx = min(max(sx + i, 0), dw - 1);
                        e[i] = wear_add(row[cx], inc | (cx != sx + i ? 1u << 16 : 0u));
                    }
                }
            }
        }
        uint8_t *o = D + ((size_t)y * dw + x) * 4;
        if (L.vec) tensor_store4<4>(o, e);
        else {
#pragma unroll
            for (int i = 0; i < 4; i++)
                if (x + i < dw) ((g_u32p)o)[i] = e[i];
        }
    }
}

template <int DTYPE>
__device__ __forceinline__ void wear_body(const uint8_t *__restrict__ pool, size_t pool_stride, uint8_t *__restrict__ dst, size_t dst_stride,
                                          const WearLaunch &L)
{
    typedef typename TensorElem<DTYPE>::T elem_t;
    constexpr int ES = (int)sizeof(elem_t);
    const int f = (int)blockIdx.y;
    const int gw = L.g.gw, gh = L.g.gh;
    int y0, y1;
    tensor_share(0, gh, L.g.S, (int)blockIdx.x, y0, y1);
    const uint8_t *src = pool + pool_stride * (size_t)L.idx[f];
    uint8_t *D = dst + dst_stride * f;
    const size_t plane = (size_t)gh * gw;
    const int nrows = y1 - y0;
#pragma unroll 1
    for (TensorWalk t((gw + 3) >> 2); t.row < nrows; t.next()) {
        const int y = y0 + t.row, x = t.col << 2;
        const TraceQuad q = trace_read4(src, L.g, y, x);
        uint8_t *o = D + ((size_t)y * gw + x) * ES;
#pragma unroll
        for (int c = 0; c < 4; c++) {
            if (!(L.planes >> c & 1u)) continue;         // (the same for every lane)
            const int v[4] = {(int)(q.T[0] >> 8 * c & 255u), (int)(q.T[1] >> 8 * c & 255u), (int)(q.T[2] >> 8 * c & 255u), (int)(q.T[3] >> 8 * c & 255u)};
            unsigned e[4];
            tensor_values4<DTYPE>(v, L.scale[c], e);
            if (L.g.vec) tensor_store4<ES>(o, e);
            else {
#pragma unroll
                for (int i = 0; i < 4; i++)
                    if (x + i < gw) ((GLOBAL_AS elem_t *)o)[i] = (elem_t)e[i];
            }
            o += plane * ES;
        }
    }
}

// grid: x = the workgroups that share a frame's output rows (L.g.S), y = the frames of the launch.  pool: entry 0; dst: the launch's
// first frame.
#define WEAR_KERNEL(NAME, DTYPE)                                                                                                          \
    extern "C" __global__ void __launch_bounds__(256)                                                                                     \
    NAME(const uint8_t *__restrict__ pool, size_t pool_stride, uint8_t *__restrict__ dst, size_t dst_stride, WearLaunch L)                \
    {                                                                                                                                     \
        wear_body<DTYPE>(pool, pool_stride, dst, dst_stride, L);                                                                          \
    }
WEAR_KERNEL(vp8_wear_u8_kernel, TENSOR_U8)
WEAR_KERNEL(vp8_wear_f16_kernel, TENSOR_F16)
WEAR_KERNEL(vp8_wear_f32_kernel, TENSOR_F32)
