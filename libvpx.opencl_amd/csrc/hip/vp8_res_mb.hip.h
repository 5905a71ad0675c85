// What the kernels that read a run of macroblock records share of their first two phases (vp8_residual.hip, vp8_coef.hip): the staged
// record's words the transform phase writes -- the segment's six factors and the mask of blocks that have 32 bytes in the stream, a
// block's offset being sparse_first + popcount(mask below k) -- and the lane per macroblock that makes them and runs the Y2 block's
// inverse WHT.
#pragma once
#include "vp8_simt_prims.hip.h"
#include "vp8hip.h"

// dwords of a staged record the transform phase writes: the record's reserved tail
#define RES_W_DQ 28                // three dwords: y1dc | y1ac << 16, y2dc | y2ac << 16, uvdc | uvac << 16
#define RES_W_MASK 31              // bit k: block k has 32 bytes in the stream (eobs[k] > 1, macroblock not skipped)

__device__ __forceinline__ int res_qi(int q, unsigned delta_byte)
{
    const int v = q + (int)(signed char)(delta_byte & 255u);
    return v < 0 ? 0 : (v > 127 ? 127 : v);
}

// phase 2, a lane per macroblock
__device__ __forceinline__ void res_macroblock(unsigned *rec, const ResSlot &hs)
{
    const u32 r0 = rec[0];
    const u32 y_mode = r0 & 255u;
    const bool skip = (r0 >> 24) & VP8IR_MB_SKIP;
    const bool has_y2 = y_mode != VP8IR_B_PRED && y_mode != VP8IR_SPLITMV;
    const int q = (int)((hs.q >> (7 * (rec[1] & 3u))) & 127u);
    // vp8cx_init_de_quantizer + mb_init_dequantizer, as segment_dequant (vp8_simt_prims.hip.h) from the launch's header bits
    const int y1dc = k_dc_q[res_qi(q, hs.d0)], y1ac = k_ac_q[q];
    const int y2dc = k_dc_q[res_qi(q, hs.d0 >> 8)] * 2;
    int y2ac = (k_ac_q[res_qi(q, hs.d0 >> 16)] * 155) / 100; if (y2ac < 8) y2ac = 8;
    int uvdc = k_dc_q[res_qi(q, hs.d0 >> 24)]; if (uvdc > 132) uvdc = 132;
    const int uvac = k_ac_q[res_qi(q, hs.d1)];
    rec[RES_W_DQ] = (u32)y1dc | ((u32)y1ac << 16);
    rec[RES_W_DQ + 1] = (u32)y2dc | ((u32)y2ac << 16);
    rec[RES_W_DQ + 2] = (u32)uvdc | ((u32)uvac << 16);
    const unsigned char *eobs = (const unsigned char *)rec + 8;
    u32 mask = 0;
    if (!skip) {
#pragma unroll
        for (int k = 0; k < 24; k++) mask |= eobs[k] > 1 ? 1u << k : 0u;
    }
    rec[RES_W_MASK] = mask;
    if (!has_y2 || skip) return;
    short *y2 = (short *)(rec + 16);
    if (eobs[24] > 1) {
        // the block is column-major: y2[col * 4 + row] is the reference's input[row * 4 + col]
        int in[16];
#pragma unroll
        for (int i = 0; i < 16; i++) in[(i & 3) * 4 + (i >> 2)] = (short)(y2[i] * (i ? y2ac : y2dc));      // vp8_dequantize_b_c
        int t[16];
#pragma unroll
        for (int c = 0; c < 4; c++) {            // idctllm.c:148-166, stored to `short output[16]`
            const int a = in[c] + in[12 + c], b = in[4 + c] + in[8 + c], cc = in[4 + c] - in[8 + c], d = in[c] - in[12 + c];
            t[c] = (short)(a + b); t[4 + c] = (short)(cc + d); t[8 + c] = (short)(a - b); t[12 + c] = (short)(d - cc);
        }
#pragma unroll
        for (int r = 0; r < 4; r++) {            // idctllm.c:171-191
            const int a = t[4 * r] + t[4 * r + 3], b = t[4 * r + 1] + t[4 * r + 2], cc = t[4 * r + 1] - t[4 * r + 2], d = t[4 * r] - t[4 * r + 3];
            y2[4 * r + 0] = (short)((a + b + 3) >> 3);
            y2[4 * r + 1] = (short)((cc + d + 3) >> 3);
            y2[4 * r + 2] = (short)((a - b + 3) >> 3);
            y2[4 * r + 3] = (short)((d - cc + 3) >> 3);
        }
    } else {
        const short a1 = (short)(((int)(short)(y2[0] * y2dc) + 3) >> 3);                                     // idctllm.c:194-204
#pragma unroll
        for (int i = 0; i < 16; i++) y2[i] = a1;
    }
}

// the 32 bytes of block k of the macroblock staged at rec, whose mask has bit k: two 16-byte pieces of the stream `blocks`
// (a slot whose entropy decode failed: garbage, read in bounds)
__device__ __forceinline__ const GLOBAL_AS u32x4 *res_block_at(const unsigned *rec, u32 mask, int k, const char *__restrict__ blocks, unsigned cap_blocks)
{
    u32 at = rec[14] + (u32)__builtin_popcount(mask & ((1u << k) - 1u));
    at = min(at, cap_blocks - 1u);
    return (const GLOBAL_AS u32x4 *)(blocks + (size_t)at * 32);
}
