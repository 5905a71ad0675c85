// The motion-compensated prediction of one macroblock by a workgroup of TFILTER_THREADS lanes, shared by the kernels that predict all
// three planes from a picture pair's vector (vp8_tfilter.hip, once per source; vp8_quant.hip, once): the reference's
// vp8_sixtap_predict16x16_c / 8x8_c, vp8_bilinear_predict16x16_c / 8x8_c and vp8_copy_mem16x16 / 8x8 over the edge-replicated coded
// area.  The caller turns a vector into the two plans (tf_plan: luma, and chroma by ITS rule for the chroma vector), then
//   tf_windows_first_pass   STAGE: the windows of E(ref_fb) the predictions can touch go to LDS as aligned dwords through frame_edge4
//           (every clamp is spent there): luma rows -2 .. 18 of the block's position at the vector's base, six dwords from the
//           aligned column at or below column -2; U and V rows -2 .. 10, four dwords each.  Only the rows the plane's path reads are
//           fetched: 16 (8) for a copy, 17 (9) for the bilinear filter, 21 (13) for the six-tap filter.  FIRST pass, from the window
//           into LDS again, four pixels an item: the six-tap row filter (sixtap_hrow_staged: two pixels a multiply, rounded and
//           clamped), the bilinear one, or for whole-pixel vectors the four bytes themselves.  A barrier behind each: every lane of
//           the workgroup calls it, and the window is read between the two only;
//   tf_owner_pred   SECOND pass, by the lane that owns four pixels of a row, from six (two, one) rows of the first pass.
// LANES.  Lane l < 64 owns the four luma pixels of block row l >> 2 at columns 4 (l & 3) ..; lanes 64 .. 79 own U, 80 .. 95 V, four
// pixels of row (l & 15) >> 1 at columns 4 (l & 1) ..: 384 pixels.  Lanes 96 .. 127 own nothing; all 128 stage and filter rows.
#pragma once
#include "vp8_frame_read.hip.h"
#include "vp8_block_prims.hip.h"

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

// STAGE and FIRST pass of one reference picture R for the plans PY (luma) and PC (chroma): win[TF_WIN] and hp[TF_H] are the
// workgroup's; two barriers, so every lane calls it or none does.  (vp8_tfilter.hip keeps these same statements written out in its
// source loop: as a call its registers are allocated differently, and its device code is held to what it was)
__device__ __forceinline__ void tf_windows_first_pass(u32 *win, u32 *hp, const HistFrame &R, const FramePlanes &L, int tid, const TfPlan &PY,
                                                      const TfPlan &PC)
{
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
}

// SECOND pass: the four predicted pixels of the owning lane (plane pl, row `row` of the block, columns 4 g ..)
__device__ __forceinline__ u32 tf_owner_pred(const u32 *hp, int pl, int row, int g, const TfPlan &PY, const TfPlan &PC)
{
    if (pl == 0) return tf_second_pass(hp + g, 4, row, PY, sixtap_taps((int)PY.oy));
    return tf_second_pass(hp + TF_H_Y + TF_H_C * (pl - 1) + g, 2, row, PC, sixtap_taps((int)PC.oy));
}
