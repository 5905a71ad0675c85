// What the decoder knows about a frame beside its pixels, as tensors in device memory (vp8hip_frames_side_async, vp8hip_side.hip;
// include/vp8hip.h has the definition): a motion vector per 4x4 block, and per block the macroblock's reference frame, mode, skip
// flag, segment and quantiser index and whether the block carries residual -- gathered from the IR slots as they lie in HBM
// (include/vp8_ir.h: vp8ir_mbx records and mvs[nmb * 16]) onto a grid of gw x gh cells:
//     output (y, x) takes luma block (by, bx) = (sy >> 2, sx >> 2), sx = ((2x + 1) * dw) / (2 * gw), sy = ((2y + 1) * dh) / (2 * gh)
// (dw x dh: the display size; for the native grid the coded size, which makes (by, bx) = (y, x)).
//
// Small input, large output.  A workgroup takes a group of R macroblock rows and the output rows whose cells lie in them (sy is
// monotone: they are one range; S workgroups share it where a grid is much taller than the frame).  It stages the first 64 bytes
// of each record -- the vp8ir_mb part -- and the rows' vectors into LDS with 16-byte loads (no vectors for a key frame: its vector
// area is stale).  Then a lane makes four neighbouring outputs of every plane and stores each four as one piece, neighbouring
// lanes contiguous (tensor_store4, vp8_tensor_out.hip.h, which also has the grid map, the walk and value x scale); with mv_vec /
// info_vec clear that tensor takes no whole pieces and every element is stored by itself (the rule is stated there).  Slot indices and the per-frame header bits travel in the kernel arguments.
// Integer and conversion arithmetic only.
#include "vp8_side_src.hip.h"      // SideCell, side_cell, side_stage: the slot-source side (shared with vp8_hist.hip)

template <int DTYPE>
__device__ __forceinline__ void side_body(const char *__restrict__ slot_base, size_t slot_bytes, size_t o_mbx, size_t o_mvs,
                                          uint8_t *__restrict__ mv_dst, size_t mv_stride, uint8_t *__restrict__ info_dst, size_t info_stride,
                                          const SideLaunch &L)
{
    typedef typename TensorElem<DTYPE>::T elem_t;
    constexpr int ES = (int)sizeof(elem_t);
    extern __shared__ __attribute__((aligned(16))) unsigned side_lds[];
    const int f = (int)blockIdx.y;
    const int gw = L.gw, gh = L.gh, cols = L.mb_cols;
    const int grp = (int)blockIdx.x / L.S, part = (int)blockIdx.x - grp * L.S;
    const int m0 = grp * L.R, m1 = min(m0 + L.R, L.mb_rows);
    int y0, y1;                                  // the output rows whose cells lie in the group's macroblock rows: this workgroup's share
    tensor_share(tensor_first(16 * m0, gh, L.dh), m1 == L.mb_rows ? gh : tensor_first(16 * m1, gh, L.dh), L.S, part, y0, y1);
    if (y0 >= y1) return;                        // (a group no output row falls into: a grid much smaller than the frame)

    const unsigned qf = L.q[f];
    const bool read_mv = mv_dst && !((qf >> 28) & 1u);
    const char *slot = slot_base + slot_bytes * (size_t)L.slot[f];
    u32x4_t *lrec = (u32x4_t *)side_lds;
    u32x4_t *lmvs = lrec + L.R * cols * 4;
    side_stage(slot, o_mbx, o_mvs, cols, m0, m1, read_mv, lrec, lmvs);
    __syncthreads();

    const unsigned *rec = (const unsigned *)lrec, *mvs = (const unsigned *)lmvs;
    uint8_t *Dm = mv_dst ? mv_dst + mv_stride * f : nullptr;
    uint8_t *Di = info_dst ? info_dst + info_stride * f : nullptr;
    const size_t plane = (size_t)gh * gw;
    const int nrows = y1 - y0;
#pragma unroll 1
    for (TensorWalk t((gw + 3) >> 2); t.row < nrows; t.next()) {
        const int y = y0 + t.row, col = t.col, x = col << 2;
        const int by = tensor_src(y, gh, L.dh) >> 2;
        const int mb_row = ((by >> 2) - m0) * cols, kr = (by & 3) * 4;
        SideCell c[4];
        if (L.xmode == SIDE_X_DISPLAY) {
            side_cell(rec, mvs, mb_row + (col >> 2), kr + (col & 3), read_mv, L.planes, qf, c[0]);
            c[1] = c[0]; c[2] = c[0]; c[3] = c[0];
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int xi = min(x + i, gw - 1);
                const int bx = L.xmode == SIDE_X_NATIVE ? xi : tensor_src(xi, gw, L.dw) >> 2;
                side_cell(rec, mvs, mb_row + (bx >> 2), kr + (bx & 3), read_mv, L.planes, qf, c[i]);
            }
        }
        const size_t pix = (size_t)y * gw + x;
        if (Dm) {
#pragma unroll
            for (int ch = 0; ch < 2; ch++) {
                unsigned e[4];
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const int v = ch == 0 ? (int)c[i].mv >> 16 : (int)(short)(c[i].mv & 0xffffu);      // x = col, y = row
                    e[i] = tensor_value<DTYPE>(v, L.scale[ch]);
                }
                uint8_t *o = Dm + ((size_t)ch * plane + pix) * ES;
                if (L.mv_vec) tensor_store4<ES>(o, e);
                else {
#pragma unroll
                    for (int i = 0; i < 4; i++)
                        if (x + i < gw) ((GLOBAL_AS elem_t *)o)[i] = (elem_t)e[i];
                }
            }
        }
        if (Di) {
            uint8_t *o = Di + pix;
#pragma unroll
            for (int b = 0; b < 6; b++) {
                if (!((L.planes >> b) & 1u)) continue;
                const unsigned e[4] = {c[0].v[b], c[1].v[b], c[2].v[b], c[3].v[b]};
                if (L.info_vec) tensor_store4<1>(o, e);
                else {
#pragma unroll
                    for (int i = 0; i < 4; i++)
                        if (x + i < gw) ((g_u8p)o)[i] = (unsigned char)e[i];
                }
                o += plane;
            }
        }
    }
}

// grid: x = the groups of macroblock rows of a frame times L.S, y = the frames of the launch.  slot_base: IR slot 0, slot_bytes
// apart, records at o_mbx and vectors at o_mvs inside; mv_dst / info_dst: the launch's first frame (either may be null).
#define SIDE_KERNEL(NAME, DTYPE)                                                                                                          \
    extern "C" __global__ void __launch_bounds__(256)                                                                                     \
    NAME(const char *__restrict__ slot_base, size_t slot_bytes, size_t o_mbx, size_t o_mvs, uint8_t *__restrict__ mv_dst, size_t mv_stride, \
         uint8_t *__restrict__ info_dst, size_t info_stride, SideLaunch L)                                                                \
    {                                                                                                                                     \
        side_body<DTYPE>(slot_base, slot_bytes, o_mbx, o_mvs, mv_dst, mv_stride, info_dst, info_stride, L);                               \
    }
SIDE_KERNEL(vp8_side_i16_kernel, TENSOR_I16)
SIDE_KERNEL(vp8_side_f16_kernel, TENSOR_F16)
SIDE_KERNEL(vp8_side_f32_kernel, TENSOR_F32)
