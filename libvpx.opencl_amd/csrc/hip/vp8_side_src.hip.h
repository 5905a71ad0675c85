// The slot-source side shared by the kernels that read what the decoder knows about a frame beside its pixels (vp8_side.hip: as
// tensors; vp8_hist.hip: as histograms): a group of macroblock rows of an IR slot staged into LDS (side_stage), and one cell -- a 4x4
// luma block -- of the staged rows as its vector and the info planes of include/vp8hip.h (side_cell): the one place that says what
// the planes REF, MODE, SKIP, SEGMENT, QINDEX and CODED are.
#pragma once
#include "vp8_tensor_out.hip.h"
#include "vp8hip.h"

struct SideCell {
    unsigned mv;                                 // row in the low half, col in the high one (vp8ir_mv)
    unsigned v[6];                               // the info planes in bit order
};

// rec: the staged records, 16 dwords each; mvs: the staged vectors, 16 dwords per macroblock; mb: the macroblock's index in the
// staged rows; k: the luma block
__device__ __forceinline__ void side_cell(const unsigned *rec, const unsigned *mvs, int mb, int k, bool read_mv, unsigned planes, unsigned qf,
                                          SideCell &c)
{
    const unsigned r0 = rec[mb * 16], seg = rec[mb * 16 + 1] & 255u;
    const unsigned y_mode = r0 & 255u, ref = (r0 >> 16) & 255u, skip = (r0 >> 24) & VP8IR_MB_SKIP;
    c.mv = read_mv && ref != VP8IR_INTRA_FRAME ? mvs[mb * 16 + k] : 0u;
    c.v[0] = ref;
    c.v[1] = y_mode;
    c.v[2] = skip;
    c.v[3] = seg;
    c.v[4] = (qf >> (7 * (seg & 3u))) & 127u;
    c.v[5] = 0;
    if (planes & (VP8HIP_SIDE_MODE | VP8HIP_SIDE_CODED)) {
        const unsigned char *b = (const unsigned char *)(rec + mb * 16);
        const unsigned eob = b[8 + k];
        const bool has_y2 = y_mode != VP8IR_B_PRED && y_mode != VP8IR_SPLITMV;
        if (y_mode == VP8IR_B_PRED) c.v[1] = 10u + b[40 + k];
        c.v[5] = skip ? 0u : eob > 1 ? 2u : (eob == 1 && !has_y2) ? 1u : 0u;          // vp8ir_block_kind for k < 16
    }
}

// Macroblock rows m0 .. m1 - 1 of the slot at `slot` (records at o_mbx, vectors at o_mvs inside it; `cols` macroblocks a row) into
// LDS with 16-byte loads: the first 64 bytes of each record -- the vp8ir_mb part -- at lrec, four pieces a macroblock, and, where
// read_mv, the rows' vectors at lmvs, four pieces a macroblock (no vectors for a key frame: its vector area is stale).  The caller
// makes the barrier.
__device__ __forceinline__ void side_stage(const char *slot, size_t o_mbx, size_t o_mvs, int cols, int m0, int m1, bool read_mv, u32x4_t *lrec,
                                           u32x4_t *lmvs)
{
    const GLOBAL_AS u32x4_t *grec = (const GLOBAL_AS u32x4_t *)(slot + o_mbx) + (size_t)m0 * cols * 8;
    const GLOBAL_AS u32x4_t *gmvs = (const GLOBAL_AS u32x4_t *)(slot + o_mvs) + (size_t)m0 * cols * 4;
    const int n = (m1 - m0) * cols * 4;          // 16-byte pieces: four of a record's eight, the four of a macroblock's vectors
#pragma unroll 1
    for (int t = threadIdx.x; t < n; t += 256) lrec[t] = grec[(t >> 2) * 8 + (t & 3)];
    if (read_mv) {
#pragma unroll 1
        for (int t = threadIdx.x; t < n; t += 256) lmvs[t] = gmvs[t];
    }
}
