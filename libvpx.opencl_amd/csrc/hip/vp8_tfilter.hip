// Motion-compensated temporal filter of pictures (vp8hip_frames_tfilter_async; vp8hip_tfilter.hip has the plan, include/vp8hip.h the
// definition): the reference's alt-ref noise reduction, vp8_temporal_filter_predictors_mb_c followed by vp8_temporal_filter_apply_c
// per source and the normalisation by cpi->fixed_divide, for all three planes.  A WORKGROUP owns one macroblock of one job and loops
// over the job's sources; nothing is shared between workgroups and nothing is added atomically: the same bits in every run.
//
// LANES.  Lane l < 64 owns the four luma pixels of block row l >> 2 at columns 4 (l & 3) ..; lanes 64 .. 79 own U, 80 .. 95 V, four
// pixels of row (l & 15) >> 1 at columns 4 (l & 1) ..: 384 outputs, each with its accumulator and count in registers across the
// sources.  Lanes 96 .. 127 own nothing; all 128 stage and filter rows.
// PER SOURCE whose weight is not 0 (a source of weight 0 is left before anything of it is fetched):
//   STAGE   the windows of E(ref_fb) the predictions can touch go to LDS as aligned dwords through frame_edge4 (every clamp is
//           spent there): luma rows -2 .. 18 of the block's position at the vector's base, six dwords from the aligned column at or
//           below column -2; U and V rows -2 .. 10, four dwords each.  Only the rows the plane's path reads are fetched: 16 (8) for
//           a copy, 17 (9) for the bilinear filter, 21 (13) for the six-tap filter.
//   FIRST   pass, from the window into LDS again, four pixels an item: the six-tap row filter (sixtap_hrow_staged: two pixels a
//           multiply, rounded and clamped), the bilinear one, or for whole-pixel vectors the four bytes themselves.
//   SECOND  pass, by the lane that owns the pixels, from six (two, one) rows of the first pass; then the blend.
// Two barriers a source: the window is read between them only, the first pass's rows behind the second only.
#include "vp8_frame_read.hip.h"
#include "vp8_block_prims.hip.h"
#include "vp8hip.h"

#define TF_WIN_Y 126              // dwords of the luma window: 21 rows of 6
#define TF_WIN_C 52               // ... of a chroma window: 13 rows of 4
#define TF_WIN (TF_WIN_Y + 2 * TF_WIN_C)
#define TF_H_Y 84                 // dwords of the first pass's luma rows: 21 rows of 4
#define TF_H_C 26                 // ... of a chroma plane's: 13 rows of 2
#define TF_H (TF_H_Y + 2 * TF_H_C)
#define TF_COPY 0                 // a plane's path for a source (the same for every lane)
#define TF_SIXTAP 1
#define TF_BILINEAR 2

// the four bytes from byte b of a staged row
__device__ __forceinline__ u32 tf_bytes4(const u32 *row, u32 b)
{
    return __builtin_amdgcn_alignbyte(row[(b >> 2) + 1], row[b >> 2], b & 3u);
}

// vp8_bilinear_filters[o] = {128 - 16 o, 16 o} with + 64 >> 7 over four pixels of a and b: (a (8 - o) + b o + 4) >> 3 gives the same
// bits, two pixels a multiply in the halves of a dword (vp8_subpel.hip's subpel_tap); offset 0 passes a through
__device__ __forceinline__ u32 tf_bil4(u32 a, u32 b, u32 o)
{
    if (o == 0u) return a;
    const u32 m = 0x00ff00ffu, r = 0x00040004u;
    const u32 even = (((a & m) * (8u - o) + (b & m) * o + r) >> 3) & m;
    const u32 odd = ((((a >> 8) & m) * (8u - o) + ((b >> 8) & m) * o + r) >> 3) & m;
    return even | odd << 8;
}

// the rows of a window (row 0 = two above the block) a path reads, for a block of n rows: [first, last)
__device__ __forceinline__ int tf_first_row(int path) { return path == TF_SIXTAP ? 0 : 2; }
__device__ __forceinline__ int tf_last_row(int path, int n) { return path == TF_SIXTAP ? n + 5 : path == TF_BILINEAR ? n + 3 : n + 2; }

// what a source's prediction of a plane is made with (the same for every lane)
struct TfPlan {
    int x, y;                     // the block's position at the vector's base, in the plane
    u32 ox, oy;                   // the offsets, 0..7
    int path;                     // TF_*
    u32 sh;                       // the byte of the window's first dword that is column x - 2
};
__device__ __forceinline__ TfPlan tf_plan(int x0, int y0, int vx, int vy, int filter)
{
    TfPlan p;
    p.x = x0 + (vx >> 3);
    p.y = y0 + (vy >> 3);
    p.ox = (u32)vx & 7u;
    p.oy = (u32)vy & 7u;
    p.path = (p.ox | p.oy) ? (filter ? TF_BILINEAR : TF_SIXTAP) : TF_COPY;
    p.sh = (u32)(p.x - 2) & 3u;
    return p;
}

template <int FORM>
__device__ __forceinline__ void tf_stage(u32 *win, const HistFrame &R, const FramePlanes &L, int tid, const TfPlan &Y, const TfPlan &C)
{
    const int xy = (Y.x - 2) & ~3, xc = (C.x - 2) & ~3;
    const int y0 = tf_first_row(Y.path), y1 = tf_last_row(Y.path, 16), c0 = tf_first_row(C.path), c1 = tf_last_row(C.path, 8);
    for (int i = tid; i < TF_WIN; i += TFILTER_THREADS) {
        if (i < TF_WIN_Y) {
            const int r = i / 6, k = i - 6 * r;
            if (r >= y0 && r < y1) win[i] = frame_edge4<FORM, 0>(R, L, xy + 4 * k, Y.y - 2 + r);
        } else {
            const int j = i - TF_WIN_Y, v = j >= TF_WIN_C, jj = j - TF_WIN_C * v, r = jj >> 2, k = jj & 3;
            if (r >= c0 && r < c1)
                win[i] = v ? frame_edge4<FORM, 2>(R, L, xc + 4 * k, C.y - 2 + r) : frame_edge4<FORM, 1>(R, L, xc + 4 * k, C.y - 2 + r);
        }
    }
}

// the first pass's four pixels at columns 4 g .. of window row r (row: that row's dwords); n: the block's rows
__device__ __forceinline__ bool tf_first_pass(u32 &out, const u32 *row, int r, int g, int n, const TfPlan &P, const SixTaps &tx)
{
    if (r < tf_first_row(P.path) || r >= tf_last_row(P.path, n)) return false;
    if (P.path == TF_SIXTAP) {
        out = sixtap_hrow_staged(row + g, P.sh, tx);
        return true;
    }
    const u32 b = P.sh + 2u + 4u * (u32)g;
    const u32 a = tf_bytes4(row, b);
    out = P.path == TF_BILINEAR ? tf_bil4(a, tf_bytes4(row, b + 1u), P.ox) : a;
    return true;
}

// the lane's four predicted pixels from the first pass's rows (h: row 0 of its columns; pitch: dwords a row)
__device__ __forceinline__ u32 tf_second_pass(const u32 *h, int pitch, int row, const TfPlan &P, const SixTaps &ty)
{
    if (P.path == TF_SIXTAP) {
        u32 H[6];
#pragma unroll
        for (int k = 0; k < 6; k++) H[k] = h[(row + k) * pitch];
        return sixtap_vcol(H, ty);
    }
    const u32 a = h[(row + 2) * pitch];
    return P.path == TF_BILINEAR ? tf_bil4(a, h[(row + 3) * pitch], P.oy) : a;
}

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
