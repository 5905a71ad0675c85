// Motion-compensated temporal filter of pictures (vp8hip_frames_tfilter_async; vp8hip_tfilter.hip has the plan, include/vp8hip.h the
// definition): the reference's alt-ref noise reduction, vp8_temporal_filter_predictors_mb_c followed by vp8_temporal_filter_apply_c
// per source and the normalisation by cpi->fixed_divide, for all three planes.  A WORKGROUP owns one macroblock of one job and loops
// over the job's sources; nothing is shared between workgroups and nothing is added atomically: the same bits in every run.
//
// LANES, STAGE, FIRST and SECOND pass of a source's prediction are vp8_mc_pred.hip.h's (shared with vp8_quant.hip).  PER SOURCE whose
// weight is not 0 (a source of weight 0 is left before anything of it is fetched): the windows, a barrier, the first pass, a barrier
// (the window is read between them only, the first pass's rows behind the second only), then the second pass by the lane that owns
// the pixels, then the blend: 384 outputs, each with its accumulator and count in registers across the sources.
#include "vp8_mc_pred.hip.h"
#include "vp8hip.h"

// vp8_temporal_filter_apply_c over the lane's four pixels: s the centre's, q the prediction's
__device__ __forceinline__ void tf_blend(u32 s, u32 q, u32 W, u32 strength, u32 round, u32 acc[4], u32 cnt[4])
{
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int sb = (int)((s >> (8 * i)) & 0xffu), qb = (int)((q >> (8 * i)) & 0xffu);
        const int d = sb - qb;
        u32 m = ((u32)(d * d) * 3u + round) >> strength;
        m = (16u - min(m, 16u)) * W;
        cnt[i] += m;
        acc[i] += m * (u32)qb;
    }
}

// grid: x = the macroblocks in raster order, y = the jobs of the launch; TFILTER_THREADS threads.  raster / tiles: frame buffer 0 in
// its two forms (vp8_scale_kernel's); mv / err: the CALL's first pair's (null where L says there is none); dst / cnt: the launch's
// first job's
extern "C" __global__ void __launch_bounds__(TFILTER_THREADS)
vp8_tfilter_frames_kernel(const uint8_t *__restrict__ raster, size_t fb_stride, const uint8_t *__restrict__ tiles, size_t tile_frame,
                          const uint8_t *__restrict__ mv, size_t mv_stride, const uint8_t *__restrict__ err, size_t err_stride,
                          uint8_t *__restrict__ dst, size_t dst_stride, uint8_t *__restrict__ cnt, size_t cnt_stride, TfilterLaunch L)
{
    __shared__ u32 win[TF_WIN], hp[TF_H];
    const int tid = (int)threadIdx.x;
    const int nmb = L.mb_cols * L.mb_rows, mb = (int)blockIdx.x;
    const int my = mb / L.mb_cols, mx = mb - my * L.mb_cols;
    const TfilterJob J = L.j[blockIdx.y];
    const HistFrame C = frame_of(raster, fb_stride, tiles, tile_frame, J.fb);

    // the lane's own pixels: plane, row and first column inside the block
    const bool owner = tid < 96;
    const int pl = tid < 64 ? 0 : 1 + ((tid - 64) >> 4);
    const int row = pl ? ((tid & 15) >> 1) : tid >> 2, g = pl ? (tid & 1) : (tid & 3);
    u32 s = 0u;
    if (owner) {
        if (pl == 0) s = frame_read4<0>(C, L, 16 * mx + 4 * g, 16 * my + row);
        else if (pl == 1) s = frame_read4<1>(C, L, 8 * mx + 4 * g, 8 * my + row);
        else s = frame_read4<2>(C, L, 8 * mx + 4 * g, 8 * my + row);
    }
    u32 acc[4] = {0u, 0u, 0u, 0u}, count[4] = {0u, 0u, 0u, 0u};
    const u32 strength = (u32)L.strength, round = strength ? 1u << (strength - 1u) : 0u;

    for (int k = 0; k < J.count; k++) {
        const size_t pair = (size_t)(J.first + k);
        // the weight and the vector: the same for every lane, and scalars, so that the barriers below are met by all or by none
        u32 W = 2u;
        if (L.err) {
            const u32 e = (u32)__builtin_amdgcn_readfirstlane((int)((const GLOBAL_AS u32 *)(err + err_stride * pair))[mb]);
            W = e < L.lo ? 2u : e < L.hi ? 1u : 0u;
        }
        if (!W) continue;
        int vx = 0, vy = 0;
        if (L.mv) {
            const GLOBAL_AS short *vp = (const GLOBAL_AS short *)(mv + mv_stride * pair);
            vx = __builtin_amdgcn_readfirstlane((int)vp[mb]);
            vy = __builtin_amdgcn_readfirstlane((int)vp[nmb + mb]);
        }
        const HistFrame R = frame_of(raster, fb_stride, tiles, tile_frame, L.ref[J.roff + k]);
        const TfPlan PY = tf_plan(16 * mx, 16 * my, vx, vy, L.filter), PC = tf_plan(8 * mx, 8 * my, vx >> 1, vy >> 1, L.filter);

        if (R.form == SCALE_FROM_RASTER) tf_stage<SCALE_FROM_RASTER>(win, R, L, tid, PY, PC);
        else if (R.form == SCALE_FROM_TILES) tf_stage<SCALE_FROM_TILES>(win, R, L, tid, PY, PC);
        else
            for (int i = tid; i < TF_WIN; i += TFILTER_THREADS) win[i] = 0u;
        __syncthreads();

        {
            const SixTaps txy = sixtap_taps((int)PY.ox), txc = sixtap_taps((int)PC.ox);
            for (int i = tid; i < TF_H; i += TFILTER_THREADS) {
                u32 v;
                if (i < TF_H_Y) {
                    if (tf_first_pass(v, win + 6 * (i >> 2), i >> 2, i & 3, 16, PY, txy)) hp[i] = v;
                } else {
                    const int j = i - TF_H_Y, p = j >= TF_H_C, jj = j - TF_H_C * p;
                    if (tf_first_pass(v, win + TF_WIN_Y + TF_WIN_C * p + 4 * (jj >> 1), jj >> 1, jj & 1, 8, PC, txc)) hp[i] = v;
                }
            }
        }
        __syncthreads();

        if (owner) {
            u32 q;
            if (pl == 0) q = tf_second_pass(hp + g, 4, row, PY, sixtap_taps((int)PY.oy));
            else q = tf_second_pass(hp + TF_H_Y + TF_H_C * (pl - 1) + g, 2, row, PC, sixtap_taps((int)PC.oy));
            tf_blend(s, q, W, strength, round, acc, count);
        }
    }
    if (!owner) return;

    // the picture and the count at the display size: the plane's origin in the packed I420 layout, then only what lies inside it
    const int cw = (L.dw + 1) >> 1, ch = (L.dh + 1) >> 1;
    const int pw = pl ? cw : L.dw, ph = pl ? ch : L.dh;
    const int x = (pl ? 8 : 16) * mx + 4 * g, y = (pl ? 8 : 16) * my + row;
    if (y >= ph) return;
    const size_t at = (pl == 0 ? (size_t)0 : (size_t)L.dw * L.dh + (pl == 2 ? (size_t)cw * ch : (size_t)0)) + (size_t)y * pw + x;
    GLOBAL_AS uint8_t *o = L.dst ? (GLOBAL_AS uint8_t *)(dst + dst_stride * blockIdx.y) + at : nullptr;
    GLOBAL_AS unsigned short *oc = L.cnt ? (GLOBAL_AS unsigned short *)(cnt + cnt_stride * blockIdx.y) + at : nullptr;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        if (x + i >= pw) break;
        const u32 n = count[i];
        if (o) o[i] = (uint8_t)(((acc[i] + (n >> 1)) * (n ? 0x80000u / n : 0u)) >> 19);      // cpi->fixed_divide[n]
        if (oc) oc[i] = (unsigned short)n;
    }
}
