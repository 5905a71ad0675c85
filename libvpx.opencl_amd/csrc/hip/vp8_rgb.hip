// Decoded frames as RGB tensors in device memory (vp8hip_frames_rgb_async, vp8hip_rgb.hip; include/vp8hip.h has the definition):
// for output pixel (x, y) of the packed I420 image S the scaler would write, Y = S.y[y][x], U = S.u[y >> 1][x >> 1], V likewise, and
//     channel = clamp255((cy * (Y - yoff) + 128 + cu * (U - 128) + cv * (V - 128)) >> 8)
// in 32-bit integers; bytes, or floats / halves from a table of the 256 values a channel can take (built in double, per workgroup).
//
// A workgroup takes a band of output rows that starts on an even row.  It stages the band's luma rows and half as many rows of U
// and V into LDS -- from the raster frame buffer or the tiles at the display size (stage_piece, shared with the scaler: 16-byte /
// 8-byte loads), or from the packed I420 image the scaler left in the call's scratch (dwords at the rows' own alignment).  Then a
// lane makes four neighbouring pixels at a time: one LDS dword of Y, two bytes each of U and V, the chroma terms once per pixel
// pair.  With vec set (width a multiple of 4, destination aligned to the piece) a lane's stores are whole pieces, neighbouring
// lanes contiguous: a piece of four elements per plane (planar: tensor_store4, vp8_tensor_out.hip.h, which also has the walk), 12
// bytes (packed bytes), 16 (four-byte pixels), 3 x 8 / 3 x 16 (packed halves / floats).  Otherwise -- odd widths, a tensor that starts on an odd byte --
// every element is stored by itself: each exactly once, none outside the frame.  The matrix, the order of the channels (folded into
// the coefficients by position) and the table are uniform arguments; layout and type are template parameters.  Integer and
// conversion arithmetic only.
#include "vp8_scale_src.hip.h"
#include "vp8_tensor_out.hip.h"

typedef unsigned int u32x3_t __attribute__((ext_vector_type(3)));
typedef unsigned int u32_any_t __attribute__((aligned(1)));
typedef u32x3_t u32x3_a4_t __attribute__((aligned(4)));

#define RGB_TABLE 768            // dwords of the value table in front of the rows (float types)

template <int DTYPE> struct RgbElem;
template <> struct RgbElem<RGB_U8> { typedef unsigned char T; };
template <> struct RgbElem<RGB_F16> { typedef unsigned short T; };
template <> struct RgbElem<RGB_F32> { typedef unsigned int T; };

// the element for byte v at position p: the byte, or the table's bits
template <int DTYPE>
__device__ __forceinline__ unsigned rgb_value(const unsigned *tab, int p, int v)
{
    if constexpr (DTYPE == RGB_U8) return (unsigned)v;
    else return tab[p * 256 + v];
}

template <int LAYOUT, int DTYPE>
__device__ __forceinline__ void rgb_body(const uint8_t *__restrict__ raster, size_t fb_stride, const uint8_t *__restrict__ tiles, size_t tile_frame,
                                         const uint8_t *__restrict__ packed, size_t packed_stride, uint8_t *__restrict__ dst, size_t dst_stride,
                                         const RgbLaunch &L)
{
    typedef typename RgbElem<DTYPE>::T elem_t;
    constexpr int ES = (int)sizeof(elem_t);
    constexpr int NC = LAYOUT == RGB_PACKED4 ? 4 : 3;
    extern __shared__ __attribute__((aligned(16))) unsigned rgb_lds[];
    const int e = L.fb[blockIdx.y];
    const int fb = e >> 2, form = e & 3;
    const int w = L.w, h = L.h;
    const int y0 = (int)blockIdx.x * L.br, y1 = min(y0 + L.br, h);
    const int nrows = y1 - y0, c0 = y0 >> 1, ncrows = ((y1 + 1) >> 1) - c0;
    const int rwy = L.p[0].rw >> 2, rwc = L.p[1].rw >> 2;           // dwords per slot
    unsigned *tab = rgb_lds;
    unsigned *ly = rgb_lds + (DTYPE == RGB_U8 ? 0 : RGB_TABLE);
    unsigned *lu = ly + L.br * rwy;
    unsigned *lv = lu + (L.br >> 1) * rwc;

    if constexpr (DTYPE != RGB_U8) {
        // (float)((double)v * scale + bias): the product is exact in double, so a fused multiply-add gives the same value
#pragma unroll 1
        for (int i = threadIdx.x; i < RGB_TABLE; i += 256) {
            const int p = i >> 8, v = i & 255;
            const float f = (float)((double)v * (double)L.scale[p] + (double)L.bias[p]);
            if constexpr (DTYPE == RGB_F32) tab[i] = __float_as_uint(f);
            else tab[i] = (unsigned)__half_as_ushort(__float2half_rn(f));
        }
    }
    if (form == SCALE_FROM_PACKED) {
        // rows of the scratch image at their own alignment: dword q of a row into dword 1 + q of its slot (the last one may run up
        // to three bytes past the row: into the next row, or into the padding behind the image)
        const GLOBAL_AS unsigned char *S = (g_cu8p)packed + packed_stride * blockIdx.y;
#pragma unroll
        for (int pl = 0; pl < 3; pl++) {
            const int pw = L.p[pl].aw, nd = (pw + 3) >> 2;
            const int r0 = pl ? c0 : y0, nr = pl ? ncrows : nrows, rwd = pl ? rwc : rwy;
            unsigned *base = pl == 0 ? ly : pl == 1 ? lu : lv;
#pragma unroll 1
            for (int t = threadIdx.x; t < nr * nd; t += 256) {
                const int k = t / nd, q = t - k * nd;
                base[k * rwd + 1 + q] = *(const GLOBAL_AS u32_any_t *)(S + L.p[pl].src_off + (size_t)(r0 + k) * pw + 4 * q);
            }
        }
    } else {
        const uint8_t *fraster = raster + fb_stride * (size_t)fb;
        const uint8_t *ftiles = tiles + tile_frame * (size_t)fb;
#pragma unroll
        for (int pl = 0; pl < 3; pl++) {
            const ScalePlane &P = L.p[pl];
            const int ps = pl ? 8 : 16;
            const int npieces = form == SCALE_FROM_TILES ? P.aw / ps + 1 : P.aw / ps;     // (tiles: the window row's extra tile)
            const int r0 = pl ? c0 : y0, nr = pl ? ncrows : nrows, rwd = pl ? rwc : rwy;
            unsigned *base = pl == 0 ? ly : pl == 1 ? lu : lv;
#pragma unroll 1
            for (int t = threadIdx.x; t < nr * npieces; t += 256) {
                const int k = t / npieces, q = t - k * npieces;
                const int r = min(r0 + k, P.ah - 1);
                if (form == SCALE_FROM_TILES && q == npieces - 1 && (r & (pl ? 7 : 15)) >= (pl ? 4 : 12)) continue;     // own rows: a piece fewer
                stage_piece(base + k * rwd, P, form, fraster, ftiles, L.mb_cols, r, q);
            }
        }
    }
    __syncthreads();

    uint8_t *D = dst + dst_stride * blockIdx.y;
    TensorWalk t((w + 3) >> 2);                                     // over the groups of four pixels in a row
    const unsigned short *lu16 = (const unsigned short *)lu, *lv16 = (const unsigned short *)lv;
#pragma unroll 1
    for (; t.row < nrows; t.next()) {
        const int row = t.row, col = t.col, x = col << 2, y = y0 + row;
        const unsigned yw = ly[row * rwy + 1 + col];
        const int ci = (row >> 1) * (rwc << 1) + 2 + col;           // (y0 is even: the band's chroma row row >> 1; 2 bytes at byte 4 + x / 2)
        const unsigned ub = lu16[ci], vb = lv16[ci];
        int c[3][4];
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int U = (int)((ub >> (8 * j)) & 255) - 128, V = (int)((vb >> (8 * j)) & 255) - 128;
#pragma unroll
            for (int p = 0; p < 3; p++) {
                const int kc = L.k0 + L.cu[p] * U + L.cv[p] * V;
#pragma unroll
                for (int i = 0; i < 2; i++) {
                    const int Y = (int)((yw >> (8 * (2 * j + i))) & 255);
                    c[p][2 * j + i] = min(max((L.cy * Y + kc) >> 8, 0), 255);
                }
            }
        }
        unsigned v[3][4];
#pragma unroll
        for (int p = 0; p < 3; p++)
#pragma unroll
            for (int i = 0; i < 4; i++) v[p][i] = rgb_value<DTYPE>(tab, p, c[p][i]);

        const size_t pix = (size_t)y * w + x;
        if (L.vec) {
            if constexpr (LAYOUT == RGB_PLANAR) {
#pragma unroll
                for (int p = 0; p < 3; p++) tensor_store4<ES>(D + ((size_t)p * h * w + pix) * ES, v[p]);
            } else if constexpr (LAYOUT == RGB_PACKED3) {
                uint8_t *o = D + pix * 3 * ES;
                if constexpr (DTYPE == RGB_U8) {
                    *(GLOBAL_AS u32x3_a4_t *)o = u32x3_t{v[0][0] | v[1][0] << 8 | v[2][0] << 16 | v[0][1] << 24,
                                                         v[1][1] | v[2][1] << 8 | v[0][2] << 16 | v[1][2] << 24,
                                                         v[2][2] | v[0][3] << 8 | v[1][3] << 16 | v[2][3] << 24};
                } else if constexpr (DTYPE == RGB_F16) {
                    ((GLOBAL_AS u32x2_t *)o)[0] = u32x2_t{v[0][0] | v[1][0] << 16, v[2][0] | v[0][1] << 16};
                    ((GLOBAL_AS u32x2_t *)o)[1] = u32x2_t{v[1][1] | v[2][1] << 16, v[0][2] | v[1][2] << 16};
                    ((GLOBAL_AS u32x2_t *)o)[2] = u32x2_t{v[2][2] | v[0][3] << 16, v[1][3] | v[2][3] << 16};
                } else {
                    ((GLOBAL_AS u32x4_t *)o)[0] = u32x4_t{v[0][0], v[1][0], v[2][0], v[0][1]};
                    ((GLOBAL_AS u32x4_t *)o)[1] = u32x4_t{v[1][1], v[2][1], v[0][2], v[1][2]};
                    ((GLOBAL_AS u32x4_t *)o)[2] = u32x4_t{v[2][2], v[0][3], v[1][3], v[2][3]};
                }
            } else {
                u32x4_t o4;
#pragma unroll
                for (int i = 0; i < 4; i++) o4[i] = v[0][i] | v[1][i] << 8 | v[2][i] << 16 | 0xff000000u;
                *(GLOBAL_AS u32x4_t *)(D + pix * 4) = o4;
            }
        } else {
            // element by element: the pixels of the group that lie in the row
            GLOBAL_AS elem_t *o = (GLOBAL_AS elem_t *)D;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                if (x + i < w) {
#pragma unroll
                    for (int p = 0; p < 3; p++) {
                        const size_t at = LAYOUT == RGB_PLANAR ? (size_t)p * h * w + pix + i : (pix + i) * NC + p;
                        o[at] = (elem_t)v[p][i];
                    }
                    if constexpr (LAYOUT == RGB_PACKED4) o[(pix + i) * 4 + 3] = (elem_t)255;
                }
            }
        }
    }
}

// grid: x = the bands of a frame, y = the frames of the launch.  raster / tiles: frame buffer 0 in its two forms (vp8_scale_kernel's);
// packed: image 0 of the scratch, packed_stride apart; dst: the launch's first frame, dst_stride apart.
#define RGB_KERNEL(NAME, LAYOUT, DTYPE)                                                                                                   \
    extern "C" __global__ void __launch_bounds__(256)                                                                                     \
    NAME(const uint8_t *__restrict__ raster, size_t fb_stride, const uint8_t *__restrict__ tiles, size_t tile_frame,                      \
         const uint8_t *__restrict__ packed, size_t packed_stride, uint8_t *__restrict__ dst, size_t dst_stride, RgbLaunch L)             \
    {                                                                                                                                     \
        rgb_body<LAYOUT, DTYPE>(raster, fb_stride, tiles, tile_frame, packed, packed_stride, dst, dst_stride, L);                         \
    }
RGB_KERNEL(vp8_rgb_planar_u8_kernel, RGB_PLANAR, RGB_U8)
RGB_KERNEL(vp8_rgb_planar_f16_kernel, RGB_PLANAR, RGB_F16)
RGB_KERNEL(vp8_rgb_planar_f32_kernel, RGB_PLANAR, RGB_F32)
RGB_KERNEL(vp8_rgb_packed3_u8_kernel, RGB_PACKED3, RGB_U8)
RGB_KERNEL(vp8_rgb_packed3_f16_kernel, RGB_PACKED3, RGB_F16)
RGB_KERNEL(vp8_rgb_packed3_f32_kernel, RGB_PACKED3, RGB_F32)
RGB_KERNEL(vp8_rgb_packed4_u8_kernel, RGB_PACKED4, RGB_U8)
