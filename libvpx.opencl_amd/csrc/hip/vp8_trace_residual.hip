// The accumulated residual (vp8hip_trace_residual_async, vp8hip_trace.hip; include/vp8hip.h has the definition): a frame minus its
// anchor picture gathered at the frame's trace, as a tensor [3][gh][gw].  Output (y, x) takes display pixel (sy, sx) by the centre map,
// the trace dword there names a position of the anchor, and the value is the difference of the two pixels' RGB bytes -- vp8_rgb.hip's
// integer conversion, once for each.
//
// vp8_anchor_*_kernel, shaped as vp8_flow_*_kernel (vp8_trace.hip): a workgroup takes a share of a job's output rows, a lane four
// neighbouring outputs at a time.  Both frame buffers are read where they lie, each in the form it has (ScaleSrc, vp8_scale_src.hip.h:
// the one place that knows the tiles), nothing staged: what a lane reads of the anchor depends on the trace.  At the display size the
// four trace dwords are one 16-byte load, the current frame's four luma bytes one dword and its chroma two bytes a plane; and where
// the four positions are neighbours in one row of the anchor -- a 4x4 block's row has one vector: the common case -- the anchor's
// luma is two aligned dwords shifted together (ScaleSrc::at4_any: the same two loads in every lane, also where the four bytes
// straddle two tiles) and its chroma the same per plane.  Anything else goes byte by byte, by coordinate.
// Stores as in vp8_trace.hip: whole pieces where the tensor allows, else element by element.
//
// THE CLAMP (vp8_trace_read.hip.h).  Here a trace value becomes an address: anchor_pos takes every one through trace_clamp, so no read
// falls outside the anchor's picture; ScaleSrc clamps to the aligned area once more.  Integer and conversion arithmetic only; no LDS.
#include "vp8_scale_src.hip.h"
#include "vp8_trace_read.hip.h"

// a frame buffer by coordinate in the form the job names (wave-uniform): plane 0 luma, 1 U, 2 V.  A frame buffer never written reads
// as zeros and no address is formed.
struct AnchorFrame {
    const uint8_t *raster, *tiles;
    int form;
};

template <int PL>
__device__ __forceinline__ ScaleSrc<SCALE_FROM_RASTER> anchor_raster(const AnchorFrame &F, const AnchorLaunch &L)
{
    const int off = PL == 0 ? L.y_off : PL == 1 ? L.u_off : L.v_off;
    return ScaleSrc<SCALE_FROM_RASTER>{(g_cu8p)(F.raster + off), PL ? L.uv_stride : L.y_stride, (PL ? L.aw >> 1 : L.aw) - 1,
                                       (PL ? L.ah >> 1 : L.ah) - 1, 0, 0, 0, 0};
}

template <int PL>
__device__ __forceinline__ ScaleSrc<SCALE_FROM_TILES> anchor_tiles(const AnchorFrame &F, const AnchorLaunch &L)
{
    // (the tile's layout as vp8_scale_kernel hands it to ScaleSrc)
    return ScaleSrc<SCALE_FROM_TILES>{(g_cu8p)F.tiles, (L.mb_cols + 1) * VP8_TILE_BYTES, (PL ? L.aw >> 1 : L.aw) - 1, (PL ? L.ah >> 1 : L.ah) - 1,
                                      PL ? 3 : 4, PL ? 4 : 12, PL ? 256 + 32 * (PL - 1) : 0, PL ? 320 + 32 * (PL - 1) : 192};
}

// HOW: 0 the byte at (x, y); 2 / 4: that many neighbouring columns from x, a multiple of it (ScaleSrc::atN); 5: four columns from any x
// (ScaleSrc::at4_any)
template <int PL, int HOW>
__device__ __forceinline__ unsigned anchor_read(const AnchorFrame &F, const AnchorLaunch &L, int x, int y)
{
    if (F.form == SCALE_FROM_RASTER) {
        const ScaleSrc<SCALE_FROM_RASTER> S = anchor_raster<PL>(F, L);
        if constexpr (HOW == 0) return (unsigned)S.at(x, y);
        else if constexpr (HOW == 5) return S.at4_any(x, y);
        else return S.template atN<HOW>(x, y);
    }
    if (F.form == SCALE_FROM_TILES) {
        const ScaleSrc<SCALE_FROM_TILES> S = anchor_tiles<PL>(F, L);
        if constexpr (HOW == 0) return (unsigned)S.at(x, y);
        else if constexpr (HOW == 5) return S.at4_any(x, y);
        else return S.template atN<HOW>(x, y);
    }
    return 0u;
}

// the position of the anchor a trace dword names
__device__ __forceinline__ void anchor_pos(unsigned t, const AnchorLaunch &L, int &ax, int &ay) { trace_clamp(t, L.g.dw, L.g.dh, ax, ay); }

// vp8_rgb.hip's conversion: the bytes at positions 0..2 of a pixel (the coefficients come by position, vp8hip_rgb_coeffs)
__device__ __forceinline__ void anchor_rgb(const AnchorLaunch &L, int Y, int U, int V, int (&c)[3])
{
    U -= 128; V -= 128;
    const int l = L.cy * Y + L.k0;
#pragma unroll
    for (int p = 0; p < 3; p++) c[p] = min(max((l + L.cu[p] * U + L.cv[p] * V) >> 8, 0), 255);
}

template <int DTYPE>
__device__ __forceinline__ void anchor_body(const uint8_t *__restrict__ raster, size_t fb_stride, const uint8_t *__restrict__ tiles, size_t tile_frame,
                                            const uint8_t *__restrict__ pool, size_t pool_stride, uint8_t *__restrict__ dst, size_t dst_stride,
                                            const AnchorLaunch &L)
{
    typedef typename TensorElem<DTYPE>::T elem_t;
    constexpr int ES = (int)sizeof(elem_t);
    const int f = (int)blockIdx.y;
    const AnchorJob J = L.j[f];
    const int gw = L.g.gw, gh = L.g.gh;
    int y0, y1;
    tensor_share(0, gh, L.g.S, (int)blockIdx.x, y0, y1);
    const AnchorFrame C{raster + fb_stride * (size_t)(J.fb >> 2), tiles + tile_frame * (size_t)(J.fb >> 2), J.fb & 3};
    const AnchorFrame A{raster + fb_stride * (size_t)(J.anchor >> 2), tiles + tile_frame * (size_t)(J.anchor >> 2), J.anchor & 3};
    const uint8_t *src = pool + pool_stride * (size_t)J.trace;
    uint8_t *D = dst + dst_stride * f;
    const size_t plane = (size_t)gh * gw;
    const int nrows = y1 - y0;
#pragma unroll 1
    for (TensorWalk t((gw + 3) >> 2); t.row < nrows; t.next()) {
        const int y = y0 + t.row, x = t.col << 2;
        // trace_read4's two paths, written out: the frame is read between the trace's loads, differently on each
        const int sy = tensor_src(y, gh, L.g.dh);
        const GLOBAL_AS unsigned *row = (const GLOBAL_AS unsigned *)src + (size_t)sy * L.g.dw;
        unsigned T[4];
        int cur[4][3], anc[4][3];
        int ax[4], ay[4];
        if (trace_whole(L.g, x)) {
            // the display size (sy = y, sx = x + i): four trace dwords, the luma dword, two chroma bytes a plane, a chroma term per pair
            const u32x4_t g = load4_dword_aligned(row + x);
            T[0] = g.x; T[1] = g.y; T[2] = g.z; T[3] = g.w;
            const unsigned yw = anchor_read<0, 4>(C, L, x, sy);
            const unsigned ub = anchor_read<1, 2>(C, L, x >> 1, sy >> 1), vb = anchor_read<2, 2>(C, L, x >> 1, sy >> 1);
#pragma unroll
            for (int i = 0; i < 4; i++)
                anchor_rgb(L, (int)((yw >> (8 * i)) & 255), (int)((ub >> (8 * (i >> 1))) & 255), (int)((vb >> (8 * (i >> 1))) & 255), cur[i]);
#pragma unroll
            for (int i = 0; i < 4; i++) anchor_pos(T[i], L, ax[i], ay[i]);
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int sx = trace_col(L.g, min(x + i, gw - 1));
                T[i] = row[sx];
                anchor_rgb(L, (int)anchor_read<0, 0>(C, L, sx, sy), (int)anchor_read<1, 0>(C, L, sx >> 1, sy >> 1),
                           (int)anchor_read<2, 0>(C, L, sx >> 1, sy >> 1), cur[i]);
                anchor_pos(T[i], L, ax[i], ay[i]);
            }
        }
        const bool run = ay[1] == ay[0] && ay[2] == ay[0] && ay[3] == ay[0] && ax[1] == ax[0] + 1 && ax[2] == ax[0] + 2 && ax[3] == ax[0] + 3;
        if (run) {
            // four neighbours in a row of the anchor: their chroma samples are the first two or three from ax[0] >> 1
            const int cx = ax[0] >> 1, cyr = ay[0] >> 1, odd = ax[0] & 1;
            const unsigned yw = anchor_read<0, 5>(A, L, ax[0], ay[0]);
            const unsigned uw = anchor_read<1, 5>(A, L, cx, cyr), vw = anchor_read<2, 5>(A, L, cx, cyr);
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int k = 8 * ((odd + i) >> 1);
                anchor_rgb(L, (int)((yw >> (8 * i)) & 255), (int)((uw >> k) & 255), (int)((vw >> k) & 255), anc[i]);
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++)
                anchor_rgb(L, (int)anchor_read<0, 0>(A, L, ax[i], ay[i]), (int)anchor_read<1, 0>(A, L, ax[i] >> 1, ay[i] >> 1),
                           (int)anchor_read<2, 0>(A, L, ax[i] >> 1, ay[i] >> 1), anc[i]);
        }
        const size_t pix = (size_t)y * gw + x;
#pragma unroll
        for (int p = 0; p < 3; p++) {
            const int a[4] = {cur[0][p] - anc[0][p], cur[1][p] - anc[1][p], cur[2][p] - anc[2][p], cur[3][p] - anc[3][p]};
            unsigned e[4];
            tensor_values4<DTYPE>(a, L.scale[p], e);
            uint8_t *o = D + ((size_t)p * plane + pix) * ES;
            if (L.g.vec) tensor_store4<ES>(o, e);
            else {
#pragma unroll
                for (int i = 0; i < 4; i++)
                    if (x + i < gw) ((GLOBAL_AS elem_t *)o)[i] = (elem_t)e[i];
            }
        }
    }
}

// grid: x = the workgroups that share a job's output rows (L.g.S), y = the jobs of the launch.  raster / tiles: frame buffer 0 in its two
// forms (vp8_scale_kernel's); pool: entry 0; dst: the launch's first frame.
#define ANCHOR_KERNEL(NAME, DTYPE)                                                                                                        \
    extern "C" __global__ void __launch_bounds__(256)                                                                                     \
    NAME(const uint8_t *__restrict__ raster, size_t fb_stride, const uint8_t *__restrict__ tiles, size_t tile_frame,                      \
         const uint8_t *__restrict__ pool, size_t pool_stride, uint8_t *__restrict__ dst, size_t dst_stride, AnchorLaunch L)              \
    {                                                                                                                                     \
        anchor_body<DTYPE>(raster, fb_stride, tiles, tile_frame, pool, pool_stride, dst, dst_stride, L);                                  \
    }
ANCHOR_KERNEL(vp8_anchor_i16_kernel, TENSOR_I16)
ANCHOR_KERNEL(vp8_anchor_f16_kernel, TENSOR_F16)
ANCHOR_KERNEL(vp8_anchor_f32_kernel, TENSOR_F32)
