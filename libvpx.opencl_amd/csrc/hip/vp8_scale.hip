// Decoded frames scaled into packed I420 in device memory: libyuv's I420Scale (third_party/libyuv/source/scale.c:3762, its C rows),
// bit for bit, from whichever form a frame buffer is in (vp8hip_frames_scale_async, vp8hip_scale.hip).
//
// The host's plan (vp8hip_scale_plan) dispatches each plane as ScalePlane (scale.c:3702) does -- copy, the exact ratios 3/4, 1/2, 3/8,
// 1/4, 1/8, and the general point-sampled / bilinear paths -- and leaves one ScalePlane per plane.  A workgroup takes a band of a
// plane's output rows: it stages the source rows each output row reads into LDS with 16-byte (chroma: 8-byte) loads, from the raster
// frame buffer or from the macroblock-window tiles a large launch leaves (vp8_detile.hip has the layout), every row clamped to the
// plane's 16-aligned area (what the reference's bordered buffer holds for every read I420Scale makes: Down38 reads up to three rows
// below the picture).  Then a lane makes aligned dwords of the destination (aligned in the address space: a tight tensor of 67x45
// frames has 4579-byte rows) out of LDS; whole dwords leave as one store, the dwords at a plane's two ends byte by byte.  The copy
// and Down34 take their bytes as LDS dwords; the other paths byte by byte.  Planes too wide for LDS are read from the frame
// directly.  Integer arithmetic only.
#include "vp8_scale_src.hip.h"      // ScaleSrc, ScaleLdsSrc, stage_piece: the frame-source side (shared with vp8_rgb.hip)

// what an output row needs of the source rows (a: first row or integer part, b: fraction or phase)
template <int PATH>
__device__ __forceinline__ int2 scale_row(const ScalePlane &P, int y)
{
    if constexpr (PATH == SCALE_COPY) return make_int2(y, 0);
    else if constexpr (PATH == SCALE_DOWN2) return make_int2(2 * y, 0);
    else if constexpr (PATH == SCALE_DOWN4) return make_int2(4 * y, 0);
    else if constexpr (PATH == SCALE_DOWN8) return make_int2(8 * y, 0);
    else if constexpr (PATH == SCALE_DOWN34) { const int g = y / 3; return make_int2(4 * g, y - 3 * g); }
    else if constexpr (PATH == SCALE_DOWN38) { const int g = y / 3, k = y - 3 * g; return make_int2(8 * g + 3 * k, k); }
    else if constexpr (PATH == SCALE_POINT) return make_int2(y * P.sh / P.dh, 0);          // ScalePlaneSimple
    else if constexpr (PATH == SCALE_BILIN8) {
        // ScalePlaneBilinear: y from 0, clamped to maxy after each step; an 8-bit row fraction
        const int yy = y == 0 ? 0 : min(y * P.dy, P.maxy);
        return make_int2(yy >> 16, (yy >> 8) & 255);
    } else {
        // ScalePlaneBilinearSimple: a half-pixel start, clamped to maxy after each step, negative positions read as 0
        const int yy = max(y == 0 ? P.y0 : min(P.y0 + y * P.dy, P.maxy), 0);
        return make_int2(yy >> 16, yy & 0xffff);
    }
}

template <class Src>
__device__ __forceinline__ int box4(const Src &S, int x, int y)       // ScaleRowDown4Int_C's element
{
    int s = 8;
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
        for (int i = 0; i < 4; i++) s += S.at(x + i, y + j);
    return s >> 4;
}

// 3 : 1 (t == 0) or 1 : 1 (t == 1) of two samples, rounded, as ScaleRowDown34_*_Int_C filters in each direction
__device__ __forceinline__ int mix34(int p, int q, int half) { return half ? (p + q + 1) >> 1 : (p * 3 + q + 2) >> 2; }

template <int PATH, bool F, class Src>
__device__ __forceinline__ int scale_px(const ScalePlane &P, const Src &S, int x, int2 r)
{
    if constexpr (PATH == SCALE_COPY) return S.at(x, r.x);
    else if constexpr (PATH == SCALE_DOWN2) {
        if constexpr (!F) return S.at(2 * x, r.x);
        else return (S.at(2 * x, r.x) + S.at(2 * x + 1, r.x) + S.at(2 * x, r.x + 1) + S.at(2 * x + 1, r.x + 1) + 2) >> 2;
    } else if constexpr (PATH == SCALE_DOWN4) {
        if constexpr (!F) return S.at(4 * x, r.x);
        else return box4(S, 4 * x, r.x);
    } else if constexpr (PATH == SCALE_DOWN8) {
        if constexpr (!F) return S.at(8 * x, r.x);
        else {
            // ScaleRowDown8Int_C: Down4Int of rows 0-3 into row[0..], of rows 4-7 into row[640..], then Down2Int with a stride of
            // 640; past 320 output pixels the second write runs over the first one's tail (element i >= 640 is the lower row's i - 640)
            const int i0 = 2 * x, i1 = 2 * x + 1;
            const int u0 = i0 < 640 ? box4(S, 4 * i0, r.x) : box4(S, 4 * (i0 - 640), r.x + 4);
            const int u1 = i1 < 640 ? box4(S, 4 * i1, r.x) : box4(S, 4 * (i1 - 640), r.x + 4);
            return (u0 + u1 + box4(S, 4 * i0, r.x + 4) + box4(S, 4 * i1, r.x + 4) + 2) >> 2;
        }
    } else if constexpr (PATH == SCALE_DOWN34) {
        const int c = x / 3, j = x - 3 * c;
        const int k = r.y;
        if constexpr (!F) return S.at(4 * c + (j == 2 ? 3 : j), r.x + (k == 2 ? 3 : k));
        else {
            // columns 0:1 3:1, 1:2 1:1, 3:2 3:1; rows the same (the third row of a group: rows 3 and 2, negative stride, scale.c:3250)
            const int xp = 4 * c + (j == 2 ? 3 : j), xq = 4 * c + (j == 0 ? 1 : 2);
            const int yp = r.x + (k == 2 ? 3 : k), yq = r.x + (k == 0 ? 1 : 2);
            return mix34(mix34(S.at(xp, yp), S.at(xq, yp), j == 1), mix34(S.at(xp, yq), S.at(xq, yq), j == 1), k == 1);
        }
    } else if constexpr (PATH == SCALE_DOWN38) {
        const int c = x / 3, j = x - 3 * c;
        const int x0 = 8 * c + 3 * j;
        if constexpr (!F) return S.at(x0, r.x);
        else {
            // ScaleRowDown38_3_Int_C / _2_Int_C: 3x3, 2x3 (last column of a group), 3x2, 2x2 boxes times 65536 / n >> 16
            const int nc = j == 2 ? 2 : 3, nr = r.y == 2 ? 2 : 3;
            int s = 0;
#pragma unroll
            for (int jj = 0; jj < 3; jj++)
#pragma unroll
                for (int ii = 0; ii < 3; ii++)
                    if (ii < nc && jj < nr) s += S.at(x0 + ii, r.x + jj);
            return (s * (65536 / (nc * nr))) >> 16;
        }
    } else if constexpr (PATH == SCALE_POINT) {
        return S.at((x * P.dx) >> 16, r.x);
    } else if constexpr (PATH == SCALE_BILIN8) {
        // ScaleFilterRows_C (8-bit fraction; element [sw] duplicates [sw - 1]), then ScaleFilterCols_C from x = 0
        const int xx = x * P.dx;
        const int xi = xx >> 16, xf = xx & 0xffff;
        const int xa = min(xi, P.sw - 1), xb = min(xi + 1, P.sw - 1);
        const int ra = (S.at(xa, r.x) * (256 - r.y) + S.at(xa, r.x + 1) * r.y) >> 8;
        const int rb = (S.at(xb, r.x) * (256 - r.y) + S.at(xb, r.x + 1) * r.y) >> 8;
        return (ra * (65536 - xf) + rb * xf) >> 16;
    } else {
        // ScalePlaneBilinearSimple: the first sample unclamped, maxx after each step
        const int xx = max(x == 0 ? P.x0 : min(P.x0 + x * P.dx, P.maxx), 0);
        const int xi = xx >> 16, xf = xx & 0xffff;
        const int r0 = (S.at(xi, r.x) * (65536 - xf) + S.at(xi + 1, r.x) * xf) >> 16;
        const int r1 = (S.at(xi, r.x + 1) * (65536 - xf) + S.at(xi + 1, r.x + 1) * xf) >> 16;
        return (r0 * (65536 - r.y) + r1 * r.y) >> 16;
    }
}

// the first source row output row y reads (its rows are lo .. lo + ScalePlane::nr - 1)
template <int PATH, bool F>
__device__ __forceinline__ int scale_lo(const ScalePlane &P, int y)
{
    const int2 r = scale_row<PATH>(P, y);
    if constexpr (PATH == SCALE_DOWN34) return r.x + (F || r.y < 2 ? r.y : 3);
    else return r.x;
}

// bytes i0 .. i1 - 1 of the window (plane pixels from (col, row) on, row by row) into acc
template <int PATH, bool F, class Src>
__device__ __forceinline__ void scale_window(const ScalePlane &P, Src S, int i0, int i1, int col, int row, unsigned &acc)
{
    S.row(row, scale_lo<PATH, F>(P, row));
    int2 r = scale_row<PATH>(P, row);
#pragma unroll
    for (int i = 0; i < SCALE_WIN; i++) {
        if (i >= i0 && i < i1) {
            acc |= (unsigned)scale_px<PATH, F, Src>(P, S, col, r) << (8 * i);
            if (++col == P.dw && i + 1 < i1) {
                col = 0;
                r = scale_row<PATH>(P, ++row);
                S.row(row, scale_lo<PATH, F>(P, row));
            }
        }
    }
}

#define SCALE_CASES(X) \
    X(SCALE_COPY, false) X(SCALE_DOWN2, false) X(SCALE_DOWN2, true) X(SCALE_DOWN4, false) X(SCALE_DOWN4, true) X(SCALE_DOWN8, false) \
    X(SCALE_DOWN8, true) X(SCALE_DOWN34, false) X(SCALE_DOWN34, true) X(SCALE_DOWN38, false) X(SCALE_DOWN38, true) X(SCALE_POINT, false) \
    X(SCALE_BILIN8, true)

template <class Src>
__device__ __forceinline__ void scale_dispatch(const ScalePlane &P, const Src &S, int i0, int i1, int col, int row, unsigned &acc)
{
    switch (P.path * 2 + P.filt) {
#define X(PATH, F) case PATH * 2 + F: scale_window<PATH, F>(P, S, i0, i1, col, row, acc); break;
    SCALE_CASES(X)
#undef X
    default: scale_window<SCALE_BILIN16, true>(P, S, i0, i1, col, row, acc); break;
    }
}

// scale_lo with the path known at run time (the staging of a band)
__device__ __forceinline__ int scale_lo_any(const ScalePlane &P, int y)
{
    switch (P.path * 2 + P.filt) {
#define X(PATH, F) case PATH * 2 + F: return scale_lo<PATH, F>(P, y);
    SCALE_CASES(X)
#undef X
    default: return scale_lo<SCALE_BILIN16, true>(P, y);
    }
}

// grid: x = the workgroups of the three planes (ScalePlane::blk0 on), y = the frames of the launch.  raster: frame buffer 0 of the
// raster pool (null when there is none), fb_stride apart; tiles: the tiled form of frame buffer 0, tile_frame apart; dst: the
// packed frame of this launch's first frame, dst_stride apart.
// A plane with a band height (ScalePlane::br) takes a workgroup per band of output rows: the band's source rows go to LDS with
// 16-byte (chroma: 8-byte) loads, then every lane makes aligned destination dwords out of LDS.  A dword belongs to the band its first
// byte lies in; the one that runs on into the next band's first row is made from the frame itself.  Planes too wide for one output
// row's source rows in 64 KB of LDS have no band height: a lane per dword, every source byte read from the frame.
extern "C" __global__ void __launch_bounds__(256)
vp8_scale_kernel(const uint8_t *__restrict__ raster, size_t fb_stride, const uint8_t *__restrict__ tiles, size_t tile_frame,
                 uint8_t *__restrict__ dst, size_t dst_stride, ScaleLaunch L)
{
    extern __shared__ unsigned scale_lds[];
    const int b = (int)blockIdx.x;
    const int pl = b >= L.p[2].blk0 ? 2 : b >= L.p[1].blk0 ? 1 : 0;
    const ScalePlane P = pl == 0 ? L.p[0] : pl == 1 ? L.p[1] : L.p[2];
    const int e = L.fb[blockIdx.y];
    const int fb = e >> 2, form = e & 3;
    const uint8_t *fraster = raster + fb_stride * (size_t)fb;
    const uint8_t *ftiles = tiles + tile_frame * (size_t)fb;
    const uintptr_t pstart = (uintptr_t)dst + dst_stride * blockIdx.y + (unsigned)P.doff, pend = pstart + (unsigned)P.dsize;
    const bool luma = P.tile_plane == 0;
    const int cp = P.tile_plane - 1;
    const ScaleSrc<SCALE_FROM_RASTER> SR{(g_cu8p)(fraster + P.src_off), P.src_stride, P.aw - 1, P.ah - 1, 0, 0, 0, 0};
    const ScaleSrc<SCALE_FROM_TILES> ST{(g_cu8p)ftiles, (L.mb_cols + 1) * VP8_TILE_BYTES, P.aw - 1, P.ah - 1,
                                        luma ? 4 : 3, luma ? 12 : 4, luma ? 0 : 256 + 32 * cp, luma ? 192 : 320 + 32 * cp};
    uintptr_t wfirst, wend;
    int y0 = 0, y1 = P.dh;
    if (P.br) {
        y0 = (b - P.blk0) * P.br;
        y1 = min(y0 + P.br, P.dh);
        // stage: slot k = (y - y0) * nr + i holds source row lo(y) + i
        const int ps = luma ? 16 : 8;
        const int npieces = form == SCALE_FROM_TILES ? P.aw / ps + 1 : P.aw / ps;     // (tiles: the window row's extra tile)
        const int nslots = (y1 - y0) * P.nr;
#pragma unroll 1
        for (int t = threadIdx.x; t < nslots * npieces; t += 256) {
            const int k = t / npieces, q = t - k * npieces;
            const int yo = k / P.nr;
            const int r = min(max(scale_lo_any(P, y0 + yo) + (k - yo * P.nr), 0), P.ah - 1);
            if (form == SCALE_FROM_TILES && q == npieces - 1 && (r & (luma ? 15 : 7)) >= (luma ? 12 : 4)) continue;   // own rows: a piece fewer
            stage_piece(scale_lds + k * (P.rw / 4), P, form, fraster, ftiles, L.mb_cols, r, q);
        }
        __syncthreads();
        const uintptr_t rs0 = pstart + (uintptr_t)y0 * (unsigned)P.dw;
        wfirst = y0 == 0 ? (pstart & ~(uintptr_t)(SCALE_WIN - 1)) : ((rs0 + SCALE_WIN - 1) & ~(uintptr_t)(SCALE_WIN - 1));
        wend = y1 == P.dh ? pend : pstart + (uintptr_t)y1 * (unsigned)P.dw;
    } else {
        wfirst = (pstart & ~(uintptr_t)(SCALE_WIN - 1)) + SCALE_WIN * (uintptr_t)(b - P.blk0) * 256;
        wend = wfirst + SCALE_WIN * 256 < pend ? wfirst + SCALE_WIN * 256 : pend;
    }
    const ScaleLdsSrc SL{(const unsigned char *)scale_lds, P.rw, P.nr, y0, 0};
    // a lane's windows lie 1024 bytes apart: one division for the first, then steps of adv_rows rows and adv_cols columns
    int row = 0, col = 0;
    {
        const uintptr_t w = wfirst + SCALE_WIN * threadIdx.x;
        const int lin = (int)((w > pstart ? w : pstart) - pstart);
        row = lin / P.dw;
        col = lin - row * P.dw;
    }
#pragma unroll 1
    for (uintptr_t win = wfirst + SCALE_WIN * threadIdx.x; win < wend; win += SCALE_WIN * 256) {
        const uintptr_t b0 = win > pstart ? win : pstart, b1 = win + SCALE_WIN < pend ? win + SCALE_WIN : pend;
        const int i0 = (int)(b0 - win), i1 = (int)(b1 - win);
        const int last = col + (i1 - i0) - 1;                          // the window's last byte: still a row of the band?
        const bool in_band = P.br && (last < P.dw || row + last / P.dw < y1);
        unsigned acc = 0;
        if (in_band && P.path == SCALE_COPY && i0 == 0 && i1 == SCALE_WIN && col + SCALE_WIN <= P.dw) {
            // the copy: the window's four bytes are neighbours in one staged row -- two aligned dwords and a byte shift
            const int a = (row - y0) * P.rw + 4 + col;
            acc = __builtin_amdgcn_alignbyte(scale_lds[(a >> 2) + 1], scale_lds[a >> 2], a & 3);
        } else if (in_band && P.path == SCALE_DOWN34 && i0 == 0 && i1 == SCALE_WIN && col + SCALE_WIN <= P.dw) {
            // Down34: four outputs take two groups of four source columns, one aligned LDS dword per group and row
            const int g = row / 3, k = row - 3 * g;
            const int c = col / 3, j0 = col - 3 * c;
            const int s0 = (row - y0) * P.nr;                         // the row's slots: lo, lo + 1 (filtered: lo = 4g + k)
            const unsigned *pp = scale_lds + (s0 + (P.filt && k == 2 ? 1 : 0)) * (P.rw / 4) + 1 + c;
            const unsigned *pq = scale_lds + (s0 + (k == 2 ? 0 : 1)) * (P.rw / 4) + 1 + c;
            const unsigned p0 = pp[0], p1 = pp[1];
            const unsigned q0 = P.filt ? pq[0] : 0u, q1 = P.filt ? pq[1] : 0u;
#pragma unroll
            for (int t = 0; t < SCALE_WIN; t++) {
                const int jt = j0 + t, jj = jt >= 3 ? jt - 3 : jt;
                const unsigned wp = jt >= 3 ? p1 : p0;
                int v;
                if (!P.filt) v = (wp >> (8 * (jj == 2 ? 3 : jj))) & 255;
                else {
                    const unsigned wq = jt >= 3 ? q1 : q0;
                    const int xp = jj == 2 ? 3 : jj, xq = jj == 0 ? 1 : 2;
                    const int hp = mix34((wp >> (8 * xp)) & 255, (wp >> (8 * xq)) & 255, jj == 1);
                    const int hq = mix34((wq >> (8 * xp)) & 255, (wq >> (8 * xq)) & 255, jj == 1);
                    v = mix34(hp, hq, k == 1);
                }
                acc |= (unsigned)v << (8 * t);
            }
        } else if (in_band) scale_dispatch(P, SL, i0, i1, col, row, acc);
        else if (form == SCALE_FROM_RASTER) scale_dispatch(P, SR, i0, i1, col, row, acc);
        else if (form == SCALE_FROM_TILES) scale_dispatch(P, ST, i0, i1, col, row, acc);
        if (i0 == 0 && i1 == SCALE_WIN) {
            *(g_u32p)win = acc;
        } else {
#pragma unroll 1
            for (int i = i0; i < i1; i++) ((g_u8p)win)[i] = (unsigned char)(acc >> (8 * i));
        }
        // the next window of this lane: 1024 bytes on (its first byte; a plane's first window may have started before the plane)
        col += P.adv_cols - (int)(b0 - win);
        row += P.adv_rows;
        while (col < 0) { col += P.dw; row--; }
        while (col >= P.dw) { col -= P.dw; row++; }
    }
}
