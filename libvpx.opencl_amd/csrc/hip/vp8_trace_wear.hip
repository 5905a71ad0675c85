// Trace wear (vp8hip_frames_wear_async and vp8hip_trace_wear_async, vp8hip_trace.hip; include/vp8hip.h has the definitions).  The
// WEAR of a frame says, for every pixel of the display-size luma grid, what happened on the way its trace took to the anchor
// picture: one dword per pixel, four saturating byte counters -- HOPS (byte 0), INTRA (1), EDGE (2), CODED (3).  An inter frame's
// wear is one hop: the pixel takes the dword the reference's wear holds where its trace went, and every byte goes up by the hop's
// 0 / 1 increment.  Wear entries live in a pool of a trace pool's geometry in the caller's device memory.
//
// vp8_wear_kernel is trace_hop_body (vp8_trace_read.hip.h has the walk; the launch is the trace's TraceLaunch) with WearHop: the LDS
// dword of a macroblock holds ref_frame in the low byte and above it the mask of the luma blocks whose CODED increment is 1, made by a
// lane per macroblock from the record's first dword, eobs[0..15] and eobs[24] (one 64-byte half line); a key frame writes zeros; and a
// pixel takes the gathered dword plus the hop's increment dword, which differs among a lane's four only in byte 2, EDGE, and only
// where the group straddles the picture's edge.
//
// vp8_wear_*_kernel is entry_tensor_body (vp8_trace_read.hip.h) with WearPlanes: a pool entry as a tensor [planes][gh][gw], each
// plane asked for holding its counter's byte.
// Integer and conversion arithmetic only; wear values are data and never become addresses.
#include "vp8_trace_read.hip.h"
#include "vp8hip.h"

// P's four byte counters plus inc's (0 or 1 each), saturating at 255: `full` has a 1 in every byte of P that is 255 (the low seven
// bits all set carries into bit 7, which P has set too), and without those increments no byte carries into its neighbour
__device__ __forceinline__ unsigned wear_add(unsigned P, unsigned inc)
{
    const unsigned full = (((P & 0x7f7f7f7fu) + 0x01010101u) & P & 0x80808080u) >> 7;
    return P + (inc & ~full);
}

struct WearHop {
    static __device__ __forceinline__ unsigned stage(const GLOBAL_AS unsigned *rec)
    {
        // vp8ir_mb: y_mode, uv_mode, ref_frame, flags in dword 0; eobs[0..15] in dwords 2..5; eobs[24] the low byte of dword 8
        const unsigned d0 = rec[0], y2 = rec[8] & 255u;
        const u32x4_t eobs = load4_dword_aligned(rec + 2);
        const unsigned y_mode = d0 & 255u;
        const bool has_y2 = y_mode != VP8IR_B_PRED && y_mode != VP8IR_SPLITMV;
        // vp8ir_block_kind(m, k) != 0: eobs[k] > 1 beside a Y2 block, eobs[k] > 0 without; vp8ir_block_kind(m, 24) != 0: all sixteen
        const unsigned least = has_y2 ? 1u : 0u;
        unsigned mask = 0;
#pragma unroll
        for (int k = 0; k < 16; k++) mask |= (((eobs[k >> 2] >> (8 * (k & 3))) & 255u) > least ? 1u : 0u) << k;
        if (has_y2 && y2) mask = 0xffffu;
        if ((d0 >> 24) & VP8IR_MB_SKIP) mask = 0;
        return ((d0 >> 16) & 255u) | mask << 8;
    }
    static __device__ __forceinline__ unsigned ref(unsigned d) { return d & 255u; }
    static __device__ __forceinline__ unsigned key(int, int, int) { return 0; }
    // HOPS, INTRA, the row's share of EDGE, CODED
    static __device__ __forceinline__ unsigned inc(unsigned d, int k, bool row_edge)
    {
        return 1u | (ref(d) == VP8IR_INTRA_FRAME ? 1u << 8 : 0u) | (row_edge ? 1u << 16 : 0u) | ((d >> (8 + k)) & 1u) << 24;
    }
    static __device__ __forceinline__ unsigned take(unsigned g, unsigned inc, bool col_edge) { return wear_add(g, inc | (col_edge ? 1u << 16 : 0u)); }
};

// grid: x = the groups of macroblock rows of a frame, y = the jobs of the launch.  slot_base: IR slot 0, slot_bytes apart, records
// at o_mbx and vectors at o_mvs inside; pool: entry 0, pool_stride apart.
extern "C" __global__ void __launch_bounds__(256)
vp8_wear_kernel(const char *__restrict__ slot_base, size_t slot_bytes, size_t o_mbx, size_t o_mvs, uint8_t *pool, size_t pool_stride, TraceLaunch L)
{
    trace_hop_body<WearHop>(slot_base, slot_bytes, o_mbx, o_mvs, pool, pool_stride, L);
}

// (WearPlanes: vp8_trace_read.hip.h, beside entry_tensor_body)
ENTRY_KERNEL(vp8_wear_u8_kernel, TENSOR_U8, WearPlanes)
ENTRY_KERNEL(vp8_wear_f16_kernel, TENSOR_F16, WearPlanes)
ENTRY_KERNEL(vp8_wear_f32_kernel, TENSOR_F32, WearPlanes)
