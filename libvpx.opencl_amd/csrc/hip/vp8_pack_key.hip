// The kernels of vp8hip_frames_pack_key_async (include/vp8hip.h has the definition, vp8hip_pack.hip the plan): compressed VP8 key
// frames from frames_intra's modes and levels.  The shape is vp8_pack.hip's, with one small pass more:
//   vp8_pack_key_plan_kernel     parallel: a lane a block finds the block's end -- from step 1 where the macroblock has a Y2 block,
//                                from step 0 where it is B_PRED -- and checks its levels; a lane a macroblock checks the modes and
//                                leaves the macroblock's record (below) in the scratch.
//   vp8_pack_key_y2_kernel       a lane a macroblock column walks the rows down and writes into every record what the Y2 context
//                                above the macroblock is: that of the nearest macroblock above it that has a Y2 block.  B_PRED
//                                macroblocks leave that context alone, so without this pass the token lane would walk up its column.
//   vp8_pack_key_first_kernel    a lane a job: the first partition behind the header the host coded (vp8hip_pack_key_header).
//   vp8_pack_key_tokens_kernel   a lane a token partition; block type, first step and the presence of Y2 are the macroblock's.
//   vp8_pack_key_assemble_kernel a workgroup a job: tag, start code, size, partitions and size table, the job's info.
// The bool coder is vp8_pack_coder.hip.h; the plan's scan and record store, the coder's start and end, the token kernel's body
// (pack_tokens<PACK_TOKENS_KEY>) and the assemble body are vp8_pack_tokens.hip.h's, shared with vp8_pack.hip and vp8_pack_adapt.hip.
//
// The record of a macroblock, eight dwords: [0] bits 0..24 "block b has a coded level" (bit 24 is 0 for B_PRED; none set: the
// macroblock is skipped), bits 25..27 the y mode, 28..29 the uv mode, bit 30 the Y2 context above (the y2 kernel's), bit 31 0;
// [1..5] the blocks' ends, five bits each, six to a dword; [6..7] the sixteen sub-block modes, four bits each -- the implied ones
// for a 16x16 mode, so a neighbour reads its contexts from here whatever the macroblock is.  Modes out of range are recorded as 0
// (and the job's status says so): no table is indexed by anything but a checked value.
#include <hip/hip_runtime.h>
#include "vp8_pack_tokens.hip.h"

#define PACK_KEY_Y2_ABOVE (1u << 30)

// ---- the plan -----------------------------------------------------------------------------------------------------------------
extern "C" __global__ __launch_bounds__(256) void vp8_pack_key_plan_kernel(const uint8_t *coef, size_t coef_stride, uint8_t *scratch, PackLaunch L, PackKey K)
{
    __shared__ uint8_t s_end[8][32];
    const int job = blockIdx.y, g = threadIdx.x >> 5, l = threadIdx.x & 31;
    const int nmb = L.mb_cols * L.mb_rows;
    const int mb = (int)blockIdx.x * 8 + g;
    const uint8_t *mode = K.modes + K.modes_stride * (size_t)job + (size_t)(mb < nmb ? mb : 0) * 32;
    const bool has_y2 = mode[0] != PACK_KEY_BPRED;
    uint32_t nz;
    bool any_bad;
    // block 24 of a B_PRED macroblock is not read; position 0 of a luma block: the Y2 block carries it where there is one
    pack_plan_scan(coef + coef_stride * (size_t)job, mb, has_y2 && l < 16 ? 1 : 0, mb < nmb && l < (has_y2 ? 25 : 24), s_end[g], nz, any_bad);
    if (l || mb >= nmb) return;

    const uint32_t *m = (const uint32_t *)mode;
    const uint32_t m0 = m[0], ym = m0 & 0xffu, uv = (m0 >> 8) & 0xffu;
    uint32_t status = any_bad ? PACK_BAD_LEVEL : 0;
    if (ym > 4 || uv > 3) status |= PACK_BAD_MODE;
    const uint32_t y = ym > 4 ? 0 : ym, u = uv > 3 ? 0 : uv;
    uint32_t sub[2] = {0, 0};
    if (y == PACK_KEY_BPRED) {
#pragma unroll
        for (int b = 0; b < 16; b++) {
            const uint32_t v = (m[1 + (b >> 2)] >> (8 * (b & 3))) & 0xffu;
            if (v > 9) status |= PACK_BAD_MODE;
            sub[b >> 3] |= (v > 9 ? 0 : v) << (4 * (b & 7));
        }
    } else {
        sub[0] = sub[1] = ((0x1320u >> (4 * y)) & 15) * 0x11111111u;    // DC: B_DC 0, V: B_VE 2, H: B_HE 3, TM: B_TM 1
    }
    uint32_t rec[8] = {nz | y << 25 | u << 28, 0, 0, 0, 0, 0, sub[0], sub[1]};
    pack_record_store(scratch, L, job, mb, rec, s_end[g], status);
    if (y == PACK_KEY_BPRED) atomicAdd(&pack_counters(scratch, job)[PACK_CTR_MODES], 1u);
}

// ---- the Y2 context above ---------------------------------------------------------------------------------------------------------
// A lane a (job, column).  A macroblock with a Y2 block leaves "its Y2 block had a coded level" (0 where it is skipped) for the
// next one below that has a Y2 block; a B_PRED macroblock, skipped or not, passes on what it got.
extern "C" __global__ __launch_bounds__(64) void vp8_pack_key_y2_kernel(uint8_t *scratch, int jobs, PackLaunch L)
{
    const int lane = (int)(blockIdx.x * 64 + threadIdx.x);
    const int job = lane / L.mb_cols, c = lane - job * L.mb_cols;
    if (job >= jobs) return;
    uint32_t *recs = (uint32_t *)pack_job(scratch, L, job);
    uint32_t above = 0;
#pragma unroll 1
    for (int r = 0; r < L.mb_rows; r++) {
        uint32_t *w = recs + (size_t)(r * L.mb_cols + c) * (PACK_RECORD_BYTES / 4);
        const uint32_t w0 = *w;
        if (above) *w = w0 | PACK_KEY_Y2_ABOVE;
        if (((w0 >> 25) & 7) != PACK_KEY_BPRED) above = (w0 >> 24) & 1;
    }
}

// ---- the first partition ----------------------------------------------------------------------------------------------------------
// A lane a job, behind the host's header: per macroblock the skip flag, the y mode down vp8_kf_ymode_tree, for B_PRED the sixteen
// sub-block modes down vp8_bmode_tree at vp8_kf_bmode_prob[above][left], the uv mode.  The 900 bytes of that table and the ten
// paths of the tree -- the indices of the probabilities along a path, a nibble each, and the bits taken -- are in LDS.
extern "C" __global__ __launch_bounds__(PACK_CODER_THREADS) void vp8_pack_key_first_kernel(uint8_t *scratch, int jobs, PackLaunch L)
{
    __shared__ uint8_t s_bmode[900];
    __shared__ uint32_t s_path[10];
    __shared__ uint8_t s_bits[10], s_len[10];
    // B_DC "0", B_TM "10", B_VE "110", B_HE "11100", B_LD "11110", B_RD "111010", B_VR "111011", B_VL "111110", B_HD "1111110", B_HU "1111111"
    constexpr uint32_t path[10] = {0x0, 0x10, 0x210, 0x43210, 0x63210, 0x543210, 0x543210, 0x763210, 0x8763210, 0x8763210};
    constexpr uint8_t bits[10] = {0x00, 0x01, 0x03, 0x07, 0x0f, 0x17, 0x37, 0x1f, 0x3f, 0x7f};
    constexpr uint8_t len[10] = {1, 2, 3, 5, 5, 6, 6, 6, 7, 7};
    for (int i = threadIdx.x; i < 900; i += PACK_CODER_THREADS) s_bmode[i] = pack_tables::vp8t_kf_bmode_probs[i];
    if (threadIdx.x < 10) {
        s_path[threadIdx.x] = path[threadIdx.x];
        s_bits[threadIdx.x] = bits[threadIdx.x];
        s_len[threadIdx.x] = len[threadIdx.x];
    }
    __syncthreads();
    const int job = (int)(blockIdx.x * PACK_CODER_THREADS + threadIdx.x);
    if (job >= jobs) return;
    uint8_t *area = pack_job(scratch, L, job);
    const int cols = L.mb_cols, nmb = L.mb_cols * L.mb_rows;
    PackCoder e = pack_coder_from_head(L.heads[L.head_of[job]], area + (size_t)nmb * PACK_RECORD_BYTES, L.first_cap);
    const uint4 *recs = (const uint4 *)area;
    const uint32_t prob_skip = (uint32_t)L.prob_skip;
    uint32_t left_hi = 0, left_lo = 0;                      // the sub-block modes of the macroblock to the left
    int c = 0;
#pragma unroll 1
    for (int mb = 0; mb < nmb; mb++) {
        const uint32_t w0 = recs[2 * mb].x;
        const uint4 hi = recs[2 * mb + 1];
        const uint32_t y = (w0 >> 25) & 7, uv = (w0 >> 28) & 3;
        if (c == 0) left_lo = left_hi = 0;                  // outside the picture: B_DC
        pack_put(e, !(w0 & PACK_NZ_MASK), prob_skip);
        if (y == PACK_KEY_BPRED) {
            pack_put(e, 0, 145);
            const uint32_t up = mb >= cols ? recs[2 * (mb - cols) + 1].w >> 16 : 0;     // blocks 12..15 of the macroblock above
            const unsigned long long own = (unsigned long long)hi.w << 32 | hi.z;
            const unsigned long long lft = (unsigned long long)left_hi << 32 | left_lo;
#pragma unroll 1
            for (int b = 0; b < 16; b++) {
                const uint32_t A = b < 4 ? (up >> (4 * b)) & 15 : (uint32_t)(own >> (4 * (b - 4))) & 15;
                const uint32_t Lm = b & 3 ? (uint32_t)(own >> (4 * (b - 1))) & 15 : (uint32_t)(lft >> (4 * (b + 3))) & 15;
                const uint32_t m = (uint32_t)(own >> (4 * b)) & 15;
                const uint8_t *pr = s_bmode + (A * 10 + Lm) * 9;
                const uint32_t idx = s_path[m], bt = s_bits[m];
                const int n = s_len[m];
#pragma unroll 1
                for (int j = 0; j < n; j++) pack_put(e, (int)(bt >> j) & 1, pr[(idx >> (4 * j)) & 15]);
            }
        } else {
            pack_put(e, 1, 145);
            pack_put(e, (int)(y >> 1), 156);
            pack_put(e, (int)(y & 1), y < 2 ? 163 : 128);
        }
        pack_put(e, uv != 0, 142);
        if (uv) {
            pack_put(e, uv > 1, 114);
            if (uv > 1) pack_put(e, (int)uv - 2, 183);
        }
        left_lo = hi.z; left_hi = hi.w;
        if (++c == cols) c = 0;
    }
    pack_first_done(e, scratch, job);
}

// ---- the token partitions -----------------------------------------------------------------------------------------------------
extern "C" __global__ __launch_bounds__(PACK_CODER_THREADS) void vp8_pack_key_tokens_kernel(const uint8_t *coef, size_t coef_stride, uint8_t *scratch, int jobs,
                                                                                           PackLaunch L)
{
    pack_tokens<PACK_TOKENS_KEY>(coef, coef_stride, scratch, jobs, L);
}

// ---- the frame ----------------------------------------------------------------------------------------------------------------
// ten bytes in front: the tag with bit 0 clear, 9d 01 2a, width and height
extern "C" __global__ __launch_bounds__(256) void vp8_pack_key_assemble_kernel(const uint8_t *scratch, uint8_t *dst, size_t dst_stride, uint32_t *info,
                                                                              PackLaunch L, PackKey K)
{
    pack_assemble<PACK_KEY_HEADER_BYTES>(
        scratch, dst, dst_stride, info, L, PACK_OVERFLOW | PACK_BAD_LEVEL | PACK_BAD_MODE,
        [](uint32_t *o, const uint32_t *ctr) {
            o[12] = ctr[PACK_CTR_MODES];    // B_PRED macroblocks
            o[13] = o[14] = o[15] = 0;
        },
        [&](uint8_t *out, uint32_t first) {
            const uint32_t tag = (uint32_t)L.version << 1 | (uint32_t)L.show_frame << 4 | first << 5;
            out[0] = (uint8_t)tag; out[1] = (uint8_t)(tag >> 8); out[2] = (uint8_t)(tag >> 16);
            out[3] = 0x9d; out[4] = 0x01; out[5] = 0x2a;
            out[6] = (uint8_t)K.width; out[7] = (uint8_t)((K.width >> 8) & 0x3f);
            out[8] = (uint8_t)K.height; out[9] = (uint8_t)((K.height >> 8) & 0x3f);
        });
}
