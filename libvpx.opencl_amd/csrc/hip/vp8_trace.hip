// Accumulated motion (vp8hip_frames_trace_async and vp8hip_trace_flow_async, vp8hip_trace.hip; include/vp8hip.h has the
// definitions).  The TRACE of a frame says, for every pixel of the display-size luma grid, which position of the anchor picture --
// the key frame that started the group -- it descends from: one dword per pixel, x' in the low int16 and y' in the high one.  An
// inter frame's trace is one hop: the pixel's vector, rounded to whole pixels and clamped to the picture, points into the reference
// its macroblock was predicted from, and the pixel takes the dword that reference's trace holds there.  Traces live in a pool in
// the caller's device memory; the references are entries of it.
//
// vp8_trace_kernel.  Small input, large output, as vp8_side.hip: a workgroup takes a group of R macroblock rows and the display rows
// inside them.  It stages what a hop reads of the slot into LDS -- the first dword of each record (y_mode, ref_frame) and the rows'
// vectors, those with 16-byte loads -- and then a lane makes four neighbouring pixels: one 4x4 block's row, so one vector, one
// reference and, where the clamp does not bite, sixteen contiguous bytes of the reference's trace, aligned to a dword only.  A key
// frame writes the identity and reads nothing.  Stores as in vp8_side.hip: whole 16-byte pieces where the pool allows, else
// element by element.  Job, references and the key-frame bit travel in the kernel arguments.
//
// vp8_flow_*_kernel.  A pool entry as a tensor [2][gh][gw]: output (y, x) takes trace pixel (sy, sx) by the centre map and holds
// T.x - sx, T.y - sy, converted as the side tensors are.
// Integer and conversion arithmetic only; trace values are data and never become addresses.
#include "vp8_trace_read.hip.h"
#include "vp8hip.h"

// grid: x = the groups of macroblock rows of a frame, y = the jobs of the launch.  slot_base: IR slot 0, slot_bytes apart, records
// at o_mbx and vectors at o_mvs inside; pool: entry 0, pool_stride apart.
extern "C" __global__ void __launch_bounds__(256)
vp8_trace_kernel(const char *__restrict__ slot_base, size_t slot_bytes, size_t o_mbx, size_t o_mvs, uint8_t *pool, size_t pool_stride, TraceLaunch L)
{
    extern __shared__ __attribute__((aligned(16))) unsigned trace_lds[];
    const TraceJob J = L.j[blockIdx.y];
    const int dw = L.dw, dh = L.dh, cols = L.mb_cols;
    const int m0 = (int)blockIdx.x * L.R, m1 = min(m0 + L.R, L.mb_rows);
    const int y0 = 16 * m0, y1 = min(16 * m1, dh);
    const bool key = J.key != 0;
    const unsigned *lrec = trace_lds + (size_t)L.R * cols * 16, *lmvs = trace_lds;        // vectors first: 16-byte pieces
    if (!key) {
        const char *slot = slot_base + slot_bytes * (size_t)J.slot;
        const GLOBAL_AS unsigned *grec = (const GLOBAL_AS unsigned *)(slot + o_mbx) + (size_t)m0 * cols * 32;
        const GLOBAL_AS u32x4_t *gmvs = (const GLOBAL_AS u32x4_t *)(slot + o_mvs) + (size_t)m0 * cols * 4;
        const int nmb = (m1 - m0) * cols;
#pragma unroll 1
        for (int t = threadIdx.x; t < nmb; t += 256) trace_lds[(size_t)L.R * cols * 16 + t] = grec[t * 32];
#pragma unroll 1
        for (int t = threadIdx.x; t < nmb * 4; t += 256) ((u32x4_t *)trace_lds)[t] = gmvs[t];
        __syncthreads();
    }

    uint8_t *D = pool + pool_stride * (size_t)J.dst;
    const int nrows = y1 - y0;
#pragma unroll 1
    for (TensorWalk t((dw + 3) >> 2); t.row < nrows; t.next()) {
        const int y = y0 + t.row, x = t.col << 2;
        const unsigned self = (unsigned)x | (unsigned)y << 16;
        unsigned e[4] = {self, self + 1, self + 2, self + 3};
        if (!key) {
            const int mb = ((y >> 4) - m0) * cols + (x >> 4);
            const unsigned ref = (lrec[mb] >> 16) & 255u;
            // an intra macroblock is held in place through the last frame
            const int pi = ref <= VP8IR_LAST_FRAME ? J.ref[0] : ref == VP8IR_GOLDEN_FRAME ? J.ref[1] : ref == VP8IR_ALTREF_FRAME ? J.ref[2] : -1;
            if (pi >= 0) {
                const unsigned v = ref == VP8IR_INTRA_FRAME ? 0u : lmvs[mb * 16 + ((y >> 2) & 3) * 4 + ((x >> 2) & 3)];
                const int dx = (((int)v >> 16) + 4) >> 3, dy = ((int)(short)(v & 0xffffu) + 4) >> 3;       // col in the high half
                const int sy = min(max(y + dy, 0), dh - 1), sx = x + dx;
                const GLOBAL_AS unsigned *row = (const GLOBAL_AS unsigned *)(pool + pool_stride * (size_t)pi) + (size_t)sy * dw;
                if (sx >= 0 && sx + 3 < dw) {
                    const u32x4_t g = load4_dword_aligned(row + sx);
                    e[0] = g.x; e[1] = g.y; e[2] = g.z; e[3] = g.w;
                } else {
#pragma unroll
                    for (int i = 0; i < 4; i++) e[i] = row[min(max(sx + i, 0), dw - 1)];
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
__device__ __forceinline__ void flow_body(const uint8_t *__restrict__ pool, size_t pool_stride, uint8_t *__restrict__ dst, size_t dst_stride,
                                          const FlowLaunch &L)
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
        const size_t pix = (size_t)y * gw + x;
#pragma unroll
        for (int ch = 0; ch < 2; ch++) {
            unsigned e[4];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int a = ch == 0 ? trace_x(q.T[i]) - q.sx[i] : trace_y(q.T[i]) - q.sy;
                e[i] = tensor_value<DTYPE>(a, L.scale[ch]);
            }
            uint8_t *o = D + ((size_t)ch * plane + pix) * ES;
            if (L.g.vec) tensor_store4<ES>(o, e);
            else {
#pragma unroll
                for (int i = 0; i < 4; i++)
                    if (x + i < gw) ((GLOBAL_AS elem_t *)o)[i] = (elem_t)e[i];
            }
        }
    }
}

// grid: x = the workgroups that share a frame's output rows (L.g.S), y = the frames of the launch.  pool: entry 0; dst: the launch's
// first frame.
#define FLOW_KERNEL(NAME, DTYPE)                                                                                                          \
    extern "C" __global__ void __launch_bounds__(256)                                                                                     \
    NAME(const uint8_t *__restrict__ pool, size_t pool_stride, uint8_t *__restrict__ dst, size_t dst_stride, FlowLaunch L)                \
    {                                                                                                                                     \
        flow_body<DTYPE>(pool, pool_stride, dst, dst_stride, L);                                                                          \
    }
FLOW_KERNEL(vp8_flow_i16_kernel, TENSOR_I16)
FLOW_KERNEL(vp8_flow_f16_kernel, TENSOR_F16)
FLOW_KERNEL(vp8_flow_f32_kernel, TENSOR_F32)
