// The transforms and the quantiser of the encoder kernels, one block held by one lane (vp8_quant.hip, vp8_intra_enc.hip): the reference's
// vp8_short_fdct4x4_c, vp8_short_walsh4x4_c, vp8_short_inv_walsh4x4_c and its two quantisers over a table staged as
// vp8hip_quant.hip's vp8hip_quant_staged_table lays it out (vp8hip_quant_table, then the three zero-bin extras).
#pragma once
#include "vp8_common.hip.h"

// offsets into a staged table, in shorts: the fields of vp8hip_quant_table, each [Y1, Y2, UV][dc, ac]
#define QT_QUANT 0
#define QT_SHIFT 6
#define QT_FAST 12
#define QT_ZBIN 18
#define QT_ROUND 24
#define QT_DEQUANT 30
#define QT_BOOST 36               // [Y1, Y2, UV][16]
#define QT_EXTRA 84               // [Y1, Y2, UV]

// vp8_short_fdct4x4_c: d = the block's residual, position 4 row + column -> o, position 4 v + u
__device__ __forceinline__ void quant_fdct(const int d[16], int o[16])
{
    int t[16];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int a1 = (d[4 * r] + d[4 * r + 3]) * 8, b1 = (d[4 * r + 1] + d[4 * r + 2]) * 8;
        const int c1 = (d[4 * r + 1] - d[4 * r + 2]) * 8, d1 = (d[4 * r] - d[4 * r + 3]) * 8;
        t[4 * r] = a1 + b1;
        t[4 * r + 2] = a1 - b1;
        t[4 * r + 1] = (c1 * 2217 + d1 * 5352 + 14500) >> 12;
        t[4 * r + 3] = (d1 * 2217 - c1 * 5352 + 7500) >> 12;
    }
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const int a1 = t[c] + t[12 + c], b1 = t[4 + c] + t[8 + c], c1 = t[4 + c] - t[8 + c], d1 = t[c] - t[12 + c];
        o[c] = (a1 + b1 + 7) >> 4;
        o[8 + c] = (a1 - b1 + 7) >> 4;
        o[4 + c] = ((c1 * 2217 + d1 * 5352 + 12000) >> 16) + (d1 != 0);
        o[12 + c] = (d1 * 2217 - c1 * 5352 + 51000) >> 16;
    }
}

// vp8_short_walsh4x4_c: d = the sixteen luma blocks' coefficient 0, position 4 block row + block column
__device__ __forceinline__ void quant_walsh(const int d[16], int o[16])
{
    int t[16];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int a1 = (d[4 * r] + d[4 * r + 2]) * 4, d1 = (d[4 * r + 1] + d[4 * r + 3]) * 4;
        const int c1 = (d[4 * r + 1] - d[4 * r + 3]) * 4, b1 = (d[4 * r] - d[4 * r + 2]) * 4;
        t[4 * r] = a1 + d1 + (a1 != 0);
        t[4 * r + 1] = b1 + c1;
        t[4 * r + 2] = b1 - c1;
        t[4 * r + 3] = a1 - d1;
    }
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const int a1 = t[c] + t[8 + c], d1 = t[4 + c] + t[12 + c], c1 = t[4 + c] - t[12 + c], b1 = t[c] - t[8 + c];
        int a2 = a1 + d1, b2 = b1 + c1, c2 = b1 - c1, d2 = a1 - d1;
        a2 += a2 < 0; b2 += b2 < 0; c2 += c2 < 0; d2 += d2 < 0;
        o[c] = (a2 + 3) >> 3;
        o[4 + c] = (b2 + 3) >> 3;
        o[8 + c] = (c2 + 3) >> 3;
        o[12 + c] = (d2 + 3) >> 3;
    }
}

// vp8_short_inv_walsh4x4_c (idctllm.c:140-192) on the dequantised Y2 block, position 4 v + u -> the sixteen luma blocks' position 0
__device__ __forceinline__ void quant_inv_walsh(const int in[16], int o[16])
{
    int t[16];
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const int a = in[c] + in[12 + c], b = in[4 + c] + in[8 + c], cc = in[4 + c] - in[8 + c], d = in[c] - in[12 + c];
        t[c] = (short)(a + b); t[4 + c] = (short)(cc + d); t[8 + c] = (short)(a - b); t[12 + c] = (short)(d - cc);
    }
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int a = t[4 * r] + t[4 * r + 3], b = t[4 * r + 1] + t[4 * r + 2], cc = t[4 * r + 1] - t[4 * r + 2], d = t[4 * r] - t[4 * r + 3];
        o[4 * r] = (short)((a + b + 3) >> 3);
        o[4 * r + 1] = (short)((cc + d + 3) >> 3);
        o[4 * r + 2] = (short)((a - b + 3) >> 3);
        o[4 * r + 3] = (short)((d - cc + 3) >> 3);
    }
}

// vp8_regular_quantize_b_c (FAST: vp8_fast_quantize_b_c) of c, position 4 v + u, with the factors of table type ty (0 Y1, 1 Y2,
// 2 UV) of the staged table T -> the levels q, the dequantised levels dq (int16 both) and the eob
template <bool FAST>
__device__ __forceinline__ int quant_scan(const int c[16], const short *T, int ty, int q[16], int dq[16])
{
    const int zz[16] = {0, 1, 4, 8, 5, 2, 3, 6, 9, 12, 13, 10, 7, 11, 14, 15};
    const short *F = T + 2 * ty;
    const int extra = T[QT_EXTRA + ty];
    const short *boost = T + QT_BOOST + 16 * ty;
    int eob = 0, run = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const int rc = zz[i], k = i ? 1 : 0;                   // (zigzag step 0 is position 0: the dc factors)
        const int z = c[rc], x = z < 0 ? -z : z;
        int y;
        if (FAST)
            y = ((x + F[QT_ROUND + k]) * F[QT_FAST + k]) >> 16;
        else {
            const int zbin = F[QT_ZBIN + k] + boost[run] + extra, xr = x + F[QT_ROUND + k];
            y = x >= zbin ? (((xr * F[QT_QUANT + k]) >> 16) + xr) >> F[QT_SHIFT + k] : 0;
            run = y ? 0 : run + 1;
        }
        const int level = z < 0 ? -y : y;
        q[rc] = level;
        dq[rc] = (short)(level * F[QT_DEQUANT + k]);
        eob = y ? i + 1 : eob;
    }
    return eob;
}
