// Transform and quantisation of the motion-compensated residual of picture pairs (vp8hip_frames_quant_async; vp8hip_quant.hip has the
// plan, include/vp8hip.h the definition): the reference's vp8_encode_inter16x16 followed by vp8_inverse_transform_mby and
// vp8_dequant_idct_add_uv_block, per macroblock.  A WORKGROUP of QUANT_THREADS lanes owns one macroblock of one job; nothing is
// shared between workgroups and nothing is added atomically: the same bits in every run.
//
// PREDICT   vp8_mc_pred.hip.h: windows through frame_edge4, first pass into LDS, second pass by the lane that owns four pixels of a
//           row (lanes 0 .. 95; its LANES paragraph).  The chroma vector is the decoder's: (c + sign) / 2, no full-pixel mask.
// RESIDUAL  the owning lane's four differences go to LDS as int16, block by block (blk: 16 entries a block, position 4 row + column).
// BLOCKS    lane b < 24 owns 4x4 block b (0..15 Y, 16..19 U, 20..23 V): both passes of vp8_short_fdct4x4_c in registers; the luma
//           lanes leave their coefficient 0 in LDS and lane 24 makes vp8_short_walsh4x4_c of the sixteen.  Lanes 0 .. 24 then scan
//           their sixteen coefficients in zigzag order (serial inside a block: the zero-run boost), from the job's table in LDS.
// INVERSE   only where rec or RECSSE is asked for: lane 24 makes the inverse Walsh transform (or its _1 form) into LDS, lanes
//           0 .. 23 dequantise and run idct_col / idct_row (or the DC-only form) and leave the sixteen values in blk; the owning
//           lanes add them to their prediction (add_clamp_pack).
// Five barriers with the inverse side, three without; every lane meets every barrier.
#include "vp8_mc_pred.hip.h"
#include "vp8_quant_prims.hip.h"
#include "vp8hip.h"

static_assert(QUANT_ERRY == VP8HIP_QUANT_ERRY && QUANT_ERRY2 == VP8HIP_QUANT_ERRY2 && QUANT_ERRUV == VP8HIP_QUANT_ERRUV, "");
static_assert(QUANT_EOBS == VP8HIP_QUANT_EOBS && QUANT_RECSSE == VP8HIP_QUANT_RECSSE, "");
static_assert(sizeof(vp8hip_quant_table) == 168 && QUANT_TABLE_SHORTS * 2 >= sizeof(vp8hip_quant_table) + 6, "");

// grid: x = the macroblocks in raster order, y = the jobs of the launch; QUANT_THREADS threads.  raster / tiles: frame buffer 0 in
// its two forms (vp8_scale_kernel's); mv and the four outputs: the launch's first job's (null where L says there is none)
extern "C" __global__ void __launch_bounds__(QUANT_THREADS)
vp8_quant_frames_kernel(const uint8_t *__restrict__ raster, size_t fb_stride, const uint8_t *__restrict__ tiles, size_t tile_frame,
                        const uint8_t *__restrict__ mv, size_t mv_stride, uint8_t *__restrict__ coef, size_t coef_stride,
                        uint8_t *__restrict__ eobs, size_t eob_stride, uint8_t *__restrict__ stats, size_t stats_stride,
                        uint8_t *__restrict__ rec, size_t rec_stride, QuantLaunch L)
{
    __shared__ u32 win[TF_WIN], hp[TF_H];
    __shared__ __attribute__((aligned(16))) short blk[24 * 16];           // the residual, later what the inverse transforms add
    __shared__ __attribute__((aligned(16))) short tab[QUANT_TABLE_SHORTS];
    __shared__ short dcs[16];                                             // the luma blocks' coefficient 0, later their Walsh DC
    __shared__ u32 red[32], sse[96];                                      // per block: its error; per owning lane: its squared error
    __shared__ __attribute__((aligned(4))) uint8_t eob8[32];
    const int tid = (int)threadIdx.x;
    const int nmb = L.mb_cols * L.mb_rows, mb = (int)blockIdx.x;
    const int my = mb / L.mb_cols, mx = mb - my * L.mb_cols;
    const QuantJob J = L.j[blockIdx.y];
    const HistFrame C = frame_of(raster, fb_stride, tiles, tile_frame, J.fb);
    const bool inverse = L.rec || (L.planes & QUANT_RECSSE);

    // the lane's own pixels: plane, row and first column inside the block; its 4x4 block and its row inside that
    const bool owner = tid < 96;
    const int pl = tid < 64 ? 0 : 1 + ((tid - 64) >> 4);
    const int row = pl ? ((tid & 15) >> 1) : tid >> 2, g = pl ? (tid & 1) : (tid & 3);
    const int at4 = 16 * (pl ? 16 + 4 * (pl - 1) + 2 * (row >> 2) + g : 4 * (row >> 2) + g) + 4 * (row & 3);
    u32 s = 0u;
    if (owner) {
        if (pl == 0) s = frame_read4<0>(C, L, 16 * mx + 4 * g, 16 * my + row);
        else if (pl == 1) s = frame_read4<1>(C, L, 8 * mx + 4 * g, 8 * my + row);
        else s = frame_read4<2>(C, L, 8 * mx + 4 * g, 8 * my + row);
    }
    if (tid < QUANT_TABLE_SHORTS / 2) ((u32 *)tab)[tid] = ((const u32 *)L.t[J.table])[tid];

    // the vector: the same for every lane, and a scalar
    int vx = 0, vy = 0;
    if (L.mv) {
        const GLOBAL_AS short *vp = (const GLOBAL_AS short *)(mv + mv_stride * blockIdx.y);
        vx = __builtin_amdgcn_readfirstlane((int)vp[mb]);
        vy = __builtin_amdgcn_readfirstlane((int)vp[nmb + mb]);
    }
    const HistFrame R = frame_of(raster, fb_stride, tiles, tile_frame, J.ref);
    const TfPlan PY = tf_plan(16 * mx, 16 * my, vx, vy, L.filter);
    const TfPlan PC = tf_plan(8 * mx, 8 * my, (vx + (vx < 0 ? -1 : 1)) / 2, (vy + (vy < 0 ? -1 : 1)) / 2, L.filter);
    tf_windows_first_pass(win, hp, R, L, tid, PY, PC);

    u32 p = 0u;
    if (owner) {
        p = tf_owner_pred(hp, pl, row, g, PY, PC);
        short4 d;
        d.x = (short)((int)(s & 0xffu) - (int)(p & 0xffu));
        d.y = (short)((int)((s >> 8) & 0xffu) - (int)((p >> 8) & 0xffu));
        d.z = (short)((int)((s >> 16) & 0xffu) - (int)((p >> 16) & 0xffu));
        d.w = (short)((int)(s >> 24) - (int)(p >> 24));
        *(short4 *)(blk + at4) = d;
    }
    __syncthreads();

    // the forward transforms
    int c[16], q[16], dq[16];
#pragma unroll
    for (int i = 0; i < 16; i++) c[i] = q[i] = dq[i] = 0;
    if (tid < 24) {
        int d[16];
#pragma unroll
        for (int i = 0; i < 16; i++) d[i] = blk[16 * tid + i];
        quant_fdct(d, c);
        if (tid < 16) dcs[tid] = (short)c[0];
    }
    __syncthreads();
    if (tid == 24) {
        int d[16];
#pragma unroll
        for (int i = 0; i < 16; i++) d[i] = dcs[i];
        quant_walsh(d, c);
    }

    // the scan, the outputs of the forward side
    int eob = 0;
    if (tid < 25) {
        const int ty = tid < 16 ? 0 : tid < 24 ? 2 : 1;
        eob = L.fast ? quant_scan<true>(c, tab, ty, q, dq) : quant_scan<false>(c, tab, ty, q, dq);
        if (L.coef) {
            const int *o = L.levels ? q : dq;
            u32x4_t lo, hi;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                lo[i] = (u32)(o[2 * i] & 0xffff) | (u32)o[2 * i + 1] << 16;
                hi[i] = (u32)(o[8 + 2 * i] & 0xffff) | (u32)o[8 + 2 * i + 1] << 16;
            }
            GLOBAL_AS u32x4_t *cp = (GLOBAL_AS u32x4_t *)(coef + coef_stride * blockIdx.y + (size_t)mb * 800 + 32 * tid);
            cp[0] = lo;
            cp[1] = hi;
        }
        if (L.planes & (QUANT_ERRY | QUANT_ERRY2 | QUANT_ERRUV)) {
            u32 e = 0u;
#pragma unroll
            for (int i = 0; i < 16; i++) {
                const int t = c[i] - dq[i];
                if (i || tid >= 16) e += (u32)(t * t);           // vp8_mbblock_error_c(mb, 1): luma without position 0
            }
            red[tid] = e;
        }
    }
    if (tid < 32) eob8[tid] = (uint8_t)eob;                      // (0 for lanes 25 .. 31)

    if (inverse) {
        if (tid == 24) {
            int w[16];
            if (eob > 1) quant_inv_walsh(dq, w);
            else {
                const int a1 = (short)((dq[0] + 3) >> 3);        // vp8_short_inv_walsh4x4_1_c
#pragma unroll
                for (int i = 0; i < 16; i++) w[i] = a1;
            }
#pragma unroll
            for (int i = 0; i < 16; i++) dcs[i] = (short)w[i];
        }
        __syncthreads();
        if (tid < 24) {
            const bool luma = tid < 16;
            const int dcf = luma ? 1 : tab[QT_DEQUANT + 4], acf = luma ? tab[QT_DEQUANT + 1] : tab[QT_DEQUANT + 5];
            const int first = luma ? dcs[tid] : q[0];
            int e = eob;
            if (luma && e == 0 && first != 0) e = 1;             // eob_adjust (both 0 and 1 take the DC-only form below)
            int r[16];
            if (e > 1) {
                int in[16], t[16];
                in[0] = (short)(first * dcf);
#pragma unroll
                for (int i = 1; i < 16; i++) in[i] = (short)(q[i] * acf);
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    int o[4];
                    idct_col(in[u], in[4 + u], in[8 + u], in[12 + u], o);
#pragma unroll
                    for (int v = 0; v < 4; v++) t[4 * v + u] = (short)o[v];
                }
#pragma unroll
                for (int v = 0; v < 4; v++) idct_row(t + 4 * v, r + 4 * v);
            } else {
                const int a1 = ((int)(short)(first * dcf) + 4) >> 3;   // vp8_dc_only_idct_add_c
#pragma unroll
                for (int i = 0; i < 16; i++) r[i] = a1;
            }
#pragma unroll
            for (int i = 0; i < 16; i++) blk[16 * tid + i] = (short)r[i];
        }
        __syncthreads();
        if (owner) {
            const short4 d = *(const short4 *)(blk + at4);
            const int r[4] = {d.x, d.y, d.z, d.w};
            p = add_clamp_pack(p, r);
            if (L.planes & QUANT_RECSSE) {
                u32 e = 0u;
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const int t = (int)((s >> (8 * i)) & 0xffu) - (int)((p >> (8 * i)) & 0xffu);
                    e += (u32)(t * t);
                }
                sse[tid] = e;
            }
        }
    }
    __syncthreads();

    if (L.eob && tid < 8) ((GLOBAL_AS u32 *)(eobs + eob_stride * blockIdx.y + (size_t)mb * 32))[tid] = ((const u32 *)eob8)[tid];
    u32 recsse = 0u;
    if ((L.planes & QUANT_RECSSE) && tid < 64) {                 // (integer sums: any order gives the same bits)
        recsse = tid < 32 ? sse[tid] + sse[tid + 32] + sse[tid + 64] : 0u;
#pragma unroll
        for (int m = 16; m; m >>= 1) recsse += (u32)__shfl_xor((int)recsse, m, 64);
    }
    if (L.planes && tid == 0) {
        GLOBAL_AS u32 *sp = (GLOBAL_AS u32 *)(stats + stats_stride * blockIdx.y) + mb;
        if (L.planes & QUANT_ERRY) {
            u32 e = 0u;
            for (int i = 0; i < 16; i++) e += red[i];
            *sp = e;
            sp += nmb;
        }
        if (L.planes & QUANT_ERRY2) {
            *sp = red[24];
            sp += nmb;
        }
        if (L.planes & QUANT_ERRUV) {
            u32 e = 0u;
            for (int i = 16; i < 24; i++) e += red[i];
            *sp = e;
            sp += nmb;
        }
        if (L.planes & QUANT_EOBS) {
            u32 e = 0u;
            for (int i = 0; i < 25; i++) e += eob8[i];
            *sp = e;
            sp += nmb;
        }
        if (L.planes & QUANT_RECSSE) *sp = recsse;
    }
    if (!owner || !L.rec) return;

    // the reconstruction at the display size: the plane's origin in the packed I420 layout, then only what lies inside it
    const int cw = (L.dw + 1) >> 1, ch = (L.dh + 1) >> 1;
    const int pw = pl ? cw : L.dw, ph = pl ? ch : L.dh;
    const int x = (pl ? 8 : 16) * mx + 4 * g, y = (pl ? 8 : 16) * my + row;
    if (y >= ph) return;
    const size_t at = (pl == 0 ? (size_t)0 : (size_t)L.dw * L.dh + (pl == 2 ? (size_t)cw * ch : (size_t)0)) + (size_t)y * pw + x;
    GLOBAL_AS uint8_t *o = (GLOBAL_AS uint8_t *)(rec + rec_stride * blockIdx.y) + at;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        if (x + i >= pw) break;
        o[i] = (uint8_t)(p >> (8 * i));
    }
}
