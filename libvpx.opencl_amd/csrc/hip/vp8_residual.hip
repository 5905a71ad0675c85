// The decoded residual of IR slots as tensors in device memory (vp8hip_frames_residual_async, vp8hip_residual.hip; include/vp8hip.h
// has the definition): what decode_macroblock adds to the prediction before the clamp, made from the slots as they lie in HBM
// (include/vp8_ir.h: vp8ir_mbx records, the block stream through d.sparse_first) with no prediction and in no order.
//
// A workgroup takes a run of up to RES_RUN macroblocks of one macroblock row and the outputs that fall into them (the grid maps
// are monotone: one range of rows, one of columns).
//   1. stage   the run's records, 128 bytes each, into LDS with 16-byte loads
//   2. transform   a lane per macroblock: the segment's six factors, the 24-bit mask of blocks that have 32 bytes in the stream,
//      and the Y2 block's inverse WHT (vp8_short_inv_walsh4x4_c / _1_c), whose sixteen DCs replace y2[] in the staged record.
//      Then a lane per block: with eob > 1 its 32 bytes at sparse_first + popcount(mask below k), two 16-byte loads, dequantised
//      and through the two passes of vp8_short_idct4x4llm_c with their int16 truncations (dequant_idct, vp8_simt_prims.hip.h);
//      otherwise (dc + 4) >> 3 from the record alone.  Sixteen int16 into the run's image in LDS: Y 16 rows, U and V 8 rows each,
//      768 bytes a macroblock (and 16 bytes of padding a row).
//   3. output  a lane makes four neighbouring outputs of a plane from the image and stores them as one piece, neighbouring lanes
//      contiguous, or -- a group of four that a run's edge cuts -- the run's own by themselves (tensor_store4, vp8_tensor_out.hip.h,
//      which also has the grid map and its inverse, the walk and value x scale).
// Integer and conversion arithmetic only.
#include "vp8_res_mb.hip.h"
#include "vp8_tensor_out.hip.h"

// rows of the image in LDS, in samples: 16 bytes of padding each, so that the four block rows of a macroblock, which a lane per
// block writes at once, fall on different banks (without it their rows lie a multiple of 128 bytes apart)
#define RES_YW (16 * RES_RUN + 8)
#define RES_CW (8 * RES_RUN + 8)
#define RES_IMG (16 * RES_YW + 16 * RES_CW)
#define RES_REC_WORDS (RES_RUN * VP8IR_MBX_WORDS)

// phase 2, a lane per block: block k of the macroblock staged at rec, which is number mb of the run
__device__ __forceinline__ void res_block(const unsigned *rec, int mb, int k, const char *__restrict__ blocks, unsigned cap_blocks, short *img)
{
    const u32 r0 = rec[0];
    const u32 y_mode = r0 & 255u;
    const bool skip = (r0 >> 24) & VP8IR_MB_SKIP;
    const bool has_y2 = y_mode != VP8IR_B_PRED && y_mode != VP8IR_SPLITMV;
    const bool luma = k < 16;
    const u32 dq = rec[RES_W_DQ + (luma ? 0 : 2)];
    const bool dc_given = luma && has_y2;        // the WHT's DC, factor 1 (decodframe.c:92)
    const int dqdc = dc_given ? 1 : (int)(dq & 0xffffu), dqac = (int)(dq >> 16);
    const int first = ((const short *)(rec + 16))[k];          // y2[16] and cdc[8] lie one behind the other
    const u32 mask = rec[RES_W_MASK];
    short *o;
    int stride;                                  // in shorts
    if (luma) { o = img + ((k >> 2) * 4) * RES_YW + mb * 16 + (k & 3) * 4; stride = RES_YW; }
    else {
        const int kb = (k - 16) & 3;
        o = img + 16 * RES_YW + (k >= 20 ? 8 * RES_CW : 0) + ((kb >> 1) * 4) * RES_CW + mb * 8 + (kb & 1) * 4;
        stride = RES_CW;
    }
    if ((mask >> k) & 1u) {
        const GLOBAL_AS u32x4 *p = res_block_at(rec, mask, k, blocks, cap_blocks);
        const u32x4 ca = p[0], cb = p[1];
        int res[16];
        dequant_idct(ca, cb, dqdc, dqac, dc_given, first, res);
#pragma unroll
        for (int r = 0; r < 4; r++)
            *(u32x2 *)(o + r * stride) = u32x2{ ((u32)res[r * 4] & 0xffffu) | ((u32)res[r * 4 + 1] << 16), ((u32)res[r * 4 + 2] & 0xffffu) | ((u32)res[r * 4 + 3] << 16) };
    } else {
        const int dc = skip ? 0 : (int)(short)(first * dqdc);  // vp8_dc_only_idct_add_c (idctllm.c:112-138)
        const u32 v = (u32)((dc + 4) >> 3) & 0xffffu, vv = v | v << 16;
#pragma unroll
        for (int r = 0; r < 4; r++) *(u32x2 *)(o + r * stride) = u32x2{ vv, vv };
    }
}

struct ResPlane {
    const short *img;                            // the plane's image in LDS, row stride `stride` shorts
    int stride, shift;                           // shift 1: chroma under a luma sample (planar layout)
    uint8_t *dst;                                // the plane in the frame's tensor
    float scale;
};

// phase 3 for the NP planes that share one grid of g_w x g_h outputs laid over d_w x d_h samples: output rows y0 .. y1 - 1, columns
// xa .. xb - 1; (row0, col0) the run's first sample in the grid's units, w x h the samples the run holds
template <int DTYPE, int NP>
__device__ __forceinline__ void res_emit(const ResPlane (&pl)[NP], int g_w, int g_h, int d_w, int d_h, int y0, int y1, int xa, int xb, int row0, int col0,
                                         int w, int h, bool vec)
{
    typedef typename TensorElem<DTYPE>::T elem_t;
    constexpr int ES = (int)sizeof(elem_t);
    if (y0 >= y1 || xa >= xb) return;
    const bool identx = g_w == d_w, identy = g_h == d_h;
    const int q0 = xa >> 2, nrows = y1 - y0;
    TensorWalk t(((xb + 3) >> 2) - q0);                             // over the groups of four outputs the columns touch
#pragma unroll 1
    for (; t.row < nrows; t.next()) {
        const int y = y0 + t.row, x = (q0 + t.col) << 2;
        const int sy = identy ? y : tensor_src(y, g_h, d_h);
        const int ly = min(max(sy - row0, 0), h - 1);
        const bool whole = x >= xa && x + 4 <= xb;
        int lx[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int xi = min(max(x + i, xa), xb - 1);
            const int sx = identx ? xi : tensor_src(xi, g_w, d_w);
            lx[i] = min(max(sx - col0, 0), w - 1);
        }
        const size_t pix = (size_t)y * g_w + x;
#pragma unroll
        for (int p = 0; p < NP; p++) {
            const short *src = pl[p].img + (ly >> pl[p].shift) * pl[p].stride;
            int v[4];
            if (identx && whole) {               // four neighbouring samples: one read (lx[0] is a multiple of 4)
                if (pl[p].shift) {
                    const u32 d = *(const u32 *)(src + (lx[0] >> 1));
                    v[0] = v[1] = sext16(d); v[2] = v[3] = hi16(d);
                } else {
                    const u32x2 d = *(const u32x2 *)(src + lx[0]);
                    v[0] = sext16(d.x); v[1] = hi16(d.x); v[2] = sext16(d.y); v[3] = hi16(d.y);
                }
            } else {
#pragma unroll
                for (int i = 0; i < 4; i++) v[i] = src[lx[i] >> pl[p].shift];
            }
            unsigned e[4];
#pragma unroll
            for (int i = 0; i < 4; i++) e[i] = tensor_value<DTYPE>(v[i], pl[p].scale);
            uint8_t *o = pl[p].dst + pix * ES;
            if (vec && whole) tensor_store4<ES>(o, e);
            else {
#pragma unroll
                for (int i = 0; i < 4; i++)
                    if (x + i >= xa && x + i < xb) ((GLOBAL_AS elem_t *)o)[i] = (elem_t)e[i];
            }
        }
    }
}

template <int DTYPE>
__device__ __forceinline__ void res_body(const char *__restrict__ slot_base, size_t slot_bytes, size_t o_mbx, size_t o_blocks, const char *__restrict__ pool,
                                         unsigned cap_blocks, uint8_t *__restrict__ dst, size_t dst_stride, const ResLaunch &L)
{
    constexpr int ES = (int)sizeof(typename TensorElem<DTYPE>::T);
    __shared__ __attribute__((aligned(16))) unsigned lrec[RES_REC_WORDS];
    __shared__ __attribute__((aligned(16))) short img[RES_IMG];
    const int f = (int)blockIdx.y;
    const int gw = L.gw, gh = L.gh, cols = L.mb_cols;
    const int run = (int)blockIdx.x / L.S, part = (int)blockIdx.x - run * L.S;
    const int m = run / L.runs, c0 = (run - m * L.runs) * RES_RUN, c1 = min(c0 + RES_RUN, cols), nmbs = c1 - c0;
    const bool last_row = m == L.mb_rows - 1, last_run = c1 == cols;
    const bool planar = L.layout == RES_PLANAR;

    // the outputs of the run: luma (planar: all three planes), and the chroma planes of the I420 layout
    int y0, y1, cy0 = 0, cy1 = 0, cxa = 0, cxb = 0;
    tensor_share(tensor_first(16 * m, gh, L.dh), last_row ? gh : tensor_first(16 * (m + 1), gh, L.dh), L.S, part, y0, y1);
    const int xa = tensor_first(16 * c0, gw, L.dw), xb = last_run ? gw : tensor_first(16 * c1, gw, L.dw);
    if (!planar) {
        tensor_share(tensor_first(8 * m, L.ch, L.dch), last_row ? L.ch : tensor_first(8 * (m + 1), L.ch, L.dch), L.S, part, cy0, cy1);
        cxa = tensor_first(8 * c0, L.cw, L.dcw);
        cxb = last_run ? L.cw : tensor_first(8 * c1, L.cw, L.dcw);
    }
    if ((y0 >= y1 || xa >= xb) && (cy0 >= cy1 || cxa >= cxb)) return;         // (no output falls into the run: a grid much smaller than the frame)

    const ResSlot hs = L.s[f];
    const char *slot = slot_base + slot_bytes * (size_t)hs.slot;
    {
        const GLOBAL_AS u32x4 *grec = (const GLOBAL_AS u32x4 *)(slot + o_mbx) + ((size_t)m * cols + c0) * 8;
        if ((int)threadIdx.x < nmbs * 8) ((u32x4 *)lrec)[threadIdx.x] = grec[threadIdx.x];
    }
    __syncthreads();
    if ((int)threadIdx.x < nmbs) res_macroblock(lrec + threadIdx.x * VP8IR_MBX_WORDS, hs);
    __syncthreads();
    {
        const char *blocks = pool ? pool : slot + o_blocks;
#pragma unroll 1
        for (int b = threadIdx.x; b < nmbs * 24; b += 256) {
            const int mb = b / 24, k = b - mb * 24;
            res_block(lrec + mb * VP8IR_MBX_WORDS, mb, k, blocks, cap_blocks, img);
        }
    }
    __syncthreads();

    uint8_t *D = dst + dst_stride * f;
    const short *iy = img, *iu = img + 16 * RES_YW, *iv = iu + 8 * RES_CW;
    if (planar) {
        const size_t plane = (size_t)gh * gw * ES;
        const ResPlane pl[3] = { { iy, RES_YW, 0, D, L.scale[0] }, { iu, RES_CW, 1, D + plane, L.scale[1] }, { iv, RES_CW, 1, D + 2 * plane, L.scale[2] } };
        res_emit<DTYPE, 3>(pl, gw, gh, L.dw, L.dh, y0, y1, xa, xb, 16 * m, 16 * c0, 16 * nmbs, 16, L.y_vec);
    } else {
        const size_t ysize = (size_t)gh * gw * ES, csize = (size_t)L.ch * L.cw * ES;
        const ResPlane py[1] = { { iy, RES_YW, 0, D, L.scale[0] } };
        const ResPlane pc[2] = { { iu, RES_CW, 0, D + ysize, L.scale[1] }, { iv, RES_CW, 0, D + ysize + csize, L.scale[2] } };
        res_emit<DTYPE, 1>(py, gw, gh, L.dw, L.dh, y0, y1, xa, xb, 16 * m, 16 * c0, 16 * nmbs, 16, L.y_vec);
        res_emit<DTYPE, 2>(pc, L.cw, L.ch, L.dcw, L.dch, cy0, cy1, cxa, cxb, 8 * m, 8 * c0, 8 * nmbs, 8, L.c_vec);
    }
}

// grid: x = the runs of a frame (mb_rows * L.runs) times L.S, y = the frames of the launch.  slot_base: IR slot 0, slot_bytes apart,
// records at o_mbx and the block stream at o_blocks inside -- or, with pool not null, every slot's blocks in the pool, counted
// from its start; cap_blocks: blocks either holds.  dst: the launch's first frame.
#define RES_KERNEL(NAME, DTYPE)                                                                                                              \
    extern "C" __global__ void __launch_bounds__(256)                                                                                        \
    NAME(const char *__restrict__ slot_base, size_t slot_bytes, size_t o_mbx, size_t o_blocks, const char *__restrict__ pool, unsigned cap_blocks, \
         uint8_t *__restrict__ dst, size_t dst_stride, ResLaunch L)                                                                          \
    {                                                                                                                                        \
        res_body<DTYPE>(slot_base, slot_bytes, o_mbx, o_blocks, pool, cap_blocks, dst, dst_stride, L);                                       \
    }
RES_KERNEL(vp8_residual_i16_kernel, TENSOR_I16)
RES_KERNEL(vp8_residual_f16_kernel, TENSOR_F16)
RES_KERNEL(vp8_residual_f32_kernel, TENSOR_F32)
