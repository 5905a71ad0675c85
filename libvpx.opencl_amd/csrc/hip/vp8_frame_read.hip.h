// The display-size planes of a frame buffer in whichever form it has, for the kernels that read pictures and make no tensor of them
// (vp8_hist.hip, vp8_ssim.hip, vp8_motion.hip, vp8_subpel.hip, vp8_tfilter.hip): the frame of a job (frame_of), a piece of sixteen columns of a row
// (hist_read16), one aligned dword of four (frame_read4) and one of a plane's coded area extended by edge replication (frame_edge4), from
// the raster form directly, from the tiles through ScaleSrc<SCALE_FROM_TILES> (vp8_scale_src.hip.h: the one place that knows the
// tiles; frame_tiles: the one place here that describes them to it); a frame buffer never written reads as zeros and no address is
// formed.  FramePlanes (vp8_common.hip.h: what the four launches begin with) says where the planes lie.
#pragma once
#include "vp8_scale_src.hip.h"

struct HistFrame {
    const uint8_t *raster, *tiles;
    int form;                                    // SCALE_FROM_* (the same for every lane)
};

// the frame a job names as fb << 2 | form (HistFrameJob), from frame buffer 0 in its two forms
__device__ __forceinline__ HistFrame frame_of(const uint8_t *raster, size_t fb_stride, const uint8_t *tiles, size_t tile_frame, int fb)
{
    return HistFrame{raster + fb_stride * (size_t)(fb >> 2), tiles + tile_frame * (size_t)(fb >> 2), fb & 3};
}

// plane PL of F's tiles (the tile's layout as vp8_scale_kernel hands it to ScaleSrc)
template <int PL>
__device__ __forceinline__ ScaleSrc<SCALE_FROM_TILES> frame_tiles(const HistFrame &F, const FramePlanes &L)
{
    return ScaleSrc<SCALE_FROM_TILES>{(g_cu8p)F.tiles, (L.mb_cols + 1) * VP8_TILE_BYTES, (PL ? 8 : 16) * L.mb_cols - 1,
                                      (PL ? 8 : 16) * L.mb_rows - 1, PL ? 3 : 4, PL ? 4 : 12, PL ? 256 + 32 * (PL - 1) : 0,
                                      PL ? 320 + 32 * (PL - 1) : 192};
}

// columns x .. x + 15 of row y of plane PL (x a multiple of 16 below the plane's width pw), low byte first
template <int PL>
__device__ __forceinline__ u32x4_t hist_read16(const HistFrame &F, const FramePlanes &L, int x, int y, int pw)
{
    u32x4_t v = {0u, 0u, 0u, 0u};
    if (F.form == SCALE_FROM_RASTER) {
        const int off = PL == 0 ? L.y_off : PL == 1 ? L.u_off : L.v_off;
        v = *(const GLOBAL_AS u32x4_t *)((g_cu8p)F.raster + off + (long)y * (PL ? L.uv_stride : L.y_stride) + x);
    } else if (F.form == SCALE_FROM_TILES) {
        const ScaleSrc<SCALE_FROM_TILES> S = frame_tiles<PL>(F, L);
#pragma unroll
        for (int i = 0; i < 4; i++)
            if (x + 4 * i < pw) v[i] = S.template atN<4>(x + 4 * i, y);     // (pw <= the aligned width, a multiple of 8: the dword is inside it)
    }
    return v;
}

// columns x .. x + 3 of row y of plane PL (x a multiple of 4, x + 3 inside the plane: inside the aligned area), low byte first
template <int PL>
__device__ __forceinline__ unsigned frame_read4(const HistFrame &F, const FramePlanes &L, int x, int y)
{
    if (F.form == SCALE_FROM_RASTER) {
        const int off = PL == 0 ? L.y_off : PL == 1 ? L.u_off : L.v_off;
        return *(g_cu32p)((g_cu8p)F.raster + off + (long)y * (PL ? L.uv_stride : L.y_stride) + x);
    }
    if (F.form == SCALE_FROM_TILES) return frame_tiles<PL>(F, L).template atN<4>(x, y);
    return 0u;
}

// columns x .. x + 3 of row y of plane PL's CODED area (luma: 16 * mb_cols x 16 * mb_rows, chroma: half that each way) extended by
// edge replication, for any row y and any multiple of 4 x, low byte first: E(y, x) = S(clamp(y), clamp(x)), by coordinate clamps --
// the raster form's borders are never read, both forms give the same bytes.  The coded width is a multiple of 16 (chroma: of 8), so
// an aligned dword lies wholly inside the area or wholly outside it (then: the row's first or last byte, four times).  FORM is F's
// (SCALE_FROM_RASTER or _TILES: the caller branches once, not per dword); one load whatever x is, and selects: nothing here diverges
template <int FORM, int PL = 0>
__device__ __forceinline__ unsigned frame_edge4(const HistFrame &F, const FramePlanes &L, int x, int y)
{
    const int aw = (PL ? 8 : 16) * L.mb_cols, ah = (PL ? 8 : 16) * L.mb_rows;
    const int xe = min(max(x, 0), aw - 4);
    y = min(max(y, 0), ah - 1);
    unsigned v;
    if constexpr (FORM == SCALE_FROM_RASTER) {
        const int off = PL == 0 ? L.y_off : PL == 1 ? L.u_off : L.v_off;
        v = *(g_cu32p)((g_cu8p)F.raster + off + (long)y * (PL ? L.uv_stride : L.y_stride) + xe);
    } else
        v = frame_tiles<PL>(F, L).template atN<4>(xe, y);
    return x < 0 ? (v & 0xffu) * 0x01010101u : x >= aw ? (v >> 24) * 0x01010101u : v;
}
