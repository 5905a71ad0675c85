// The frame-source side shared by the kernels that read decoded frames (vp8_scale.hip, vp8_rgb.hip row by row, vp8_trace_residual.hip
// by coordinate): a plane of a frame buffer in either of its forms by coordinate (ScaleSrc), a band of source rows in LDS
// (ScaleLdsSrc), and the staging of one source row into an LDS slot with 16-byte (chroma: 8-byte) loads (stage_piece).
#pragma once
#include "vp8_common.hip.h"

typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));

// a plane of one frame buffer in one of its two forms
template <int FORM>
struct ScaleSrc {
    g_cu8p base;
    int stride;                 // raster: row stride; tiles: bytes per macroblock row of tiles
    int aw1, ah1;               // the aligned area's last column / row
    int lg, wr, wbase, obase;   // tiles: log2 macroblock size, window rows, offsets of the window / own rows in a tile

    __device__ __forceinline__ void row(int, int) {}

    // byte offset of (x, y), clamped to the aligned area
    __device__ __forceinline__ int off(int x, int y) const
    {
        x = min(max(x, 0), aw1);
        y = min(max(y, 0), ah1);
        if constexpr (FORM == SCALE_FROM_RASTER) {
            return y * stride + x;
        } else {
            // rows 0..wr-1 of a tile hold the macroblock's window (columns shifted left by 4), the rest its own columns
            const int m = (1 << lg) - 1;
            const int r = y >> lg, ry = y & m;
            const bool win = ry < wr;
            const int xx = win ? x + 4 : x;
            const int o = (win ? wbase + (ry << lg) : obase + ((ry - wr) << lg)) + (xx & m);
            return r * stride + (xx >> lg) * VP8_TILE_BYTES + o;
        }
    }

    __device__ __forceinline__ int at(int x, int y) const { return base[off(x, y)]; }

    // N = 2 or 4 neighbouring columns of row y from column x as one load, low byte first.  x is a multiple of N and x + N - 1 lies
    // inside the aligned area: such columns never leave a tile row, the window's shift by 4 included, and the load is aligned
    template <int N>
    __device__ __forceinline__ unsigned atN(int x, int y) const
    {
        if constexpr (N == 4) return *(g_cu32p)(base + off(x, y));
        else return *(const GLOBAL_AS unsigned short *)(base + off(x, y));
    }

    // four neighbouring columns of row y from ANY column x, low byte first: the aligned dword that holds column x and the one that
    // holds column x + 3 -- the same one, or the next in the row or in the next tile's row; an aligned dword never leaves a row
    // piece, the window's shift by 4 included --, shifted together.  Both addresses are clamped as at() clamps: a column past the
    // aligned area yields a byte of the area, never a read outside it.  The same in every lane whatever x is: no lane falls
    // back to bytes where four columns straddle two tiles
    __device__ __forceinline__ unsigned at4_any(int x, int y) const
    {
        const int o = off(x, y);
        const unsigned lo = *(g_cu32p)(base + (o & ~3)), hi = *(g_cu32p)(base + (off(x + 3, y) & ~3));
        return __builtin_amdgcn_alignbyte(hi, lo, (unsigned)o & 3u);
    }
};

// A band's source rows in LDS: output row y of the band has the slots (y - y0) * nr .. + nr - 1, which hold its source rows lo .. lo + nr - 1
// (clamped to the aligned area), each as columns -4 .. rw - 5 (the aligned area's columns start at byte 4 of a slot).  No column
// clamp: every path reads columns 0 .. aw - 1 only (Down* and the copy inside the picture, the bilinear rows clamp their own, the
// 16-bit one reads column 1 of a one-pixel-wide plane at most).
struct ScaleLdsSrc {
    const unsigned char *lds;
    int rw, nr, y0;
    int base;                    // of the output row being made: (its first slot - its first source row) * rw + 4

    __device__ __forceinline__ void row(int y, int first) { base = ((y - y0) * nr - first) * rw + 4; }
    __device__ __forceinline__ int at(int x, int y) const { return lds[base + y * rw + x]; }
};

// stage source row r (clamped) of the frame into an LDS slot: luma in 16-byte pieces, chroma in 8-byte pieces, from either form;
// piece q of npieces.  A tile row's window rows hold columns -4 .. 11 of the macroblock, its own rows columns 0 .. 15 (vp8_detile.hip).
__device__ __forceinline__ void stage_piece(unsigned *slot, const ScalePlane &P, int form, const uint8_t *raster, const uint8_t *tiles, int cols,
                                            int r, int q)
{
    const bool luma = P.tile_plane == 0;
    const int ps = luma ? 16 : 8;
    u32x4_t v = {0u, 0u, 0u, 0u};
    int col = q * ps;                                               // first column of the piece
    if (form == SCALE_FROM_RASTER) {
        const GLOBAL_AS unsigned char *p = (g_cu8p)raster + P.src_off + (long)r * P.src_stride + col;
        if (luma) v = *(const GLOBAL_AS u32x4_t *)p;
        else { const u32x2_t w = *(const GLOBAL_AS u32x2_t *)p; v.x = w.x; v.y = w.y; }
    } else if (form == SCALE_FROM_TILES) {
        const int lg = luma ? 4 : 3, m = (1 << lg) - 1, wr = luma ? 12 : 4, cp = P.tile_plane - 1;
        const int R = r >> lg, ry = r & m;
        const bool win = ry < wr;
        const int off = win ? (luma ? 0 : 256 + 32 * cp) + (ry << lg) : (luma ? 192 : 320 + 32 * cp) + ((ry - wr) << lg);
        const GLOBAL_AS unsigned char *p = (g_cu8p)tiles + ((long)R * (cols + 1) + q) * VP8_TILE_BYTES + off;
        if (luma) v = *(const GLOBAL_AS u32x4_t *)p;
        else { const u32x2_t w = *(const GLOBAL_AS u32x2_t *)p; v.x = w.x; v.y = w.y; }
        if (win) col -= 4;
    }
    unsigned *d = slot + (4 + col) / 4;
    d[0] = v.x;
    d[1] = v.y;
    if (luma) { d[2] = v.z; d[3] = v.w; }
}
