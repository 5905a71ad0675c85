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
// The bool coder is vp8_pack_coder.hip.h as it stands; vp8_pack_coders.inc and the kernels made from it are not touched.
//
// The record of a macroblock, eight dwords: [0] bits 0..24 "block b has a coded level" (bit 24 is 0 for B_PRED; none set: the
// macroblock is skipped), bits 25..27 the y mode, 28..29 the uv mode, bit 30 the Y2 context above (the y2 kernel's), bit 31 0;
// [1..5] the blocks' ends, five bits each, six to a dword; [6..7] the sixteen sub-block modes, four bits each -- the implied ones
// for a 16x16 mode, so a neighbour reads its contexts from here whatever the macroblock is.  Modes out of range are recorded as 0
// (and the job's status says so): no table is indexed by anything but a checked value.
#include <hip/hip_runtime.h>
#include "vp8_pack_coder.hip.h"

#define PACK_KEY_BPRED 4
#define PACK_KEY_Y2_ABOVE (1u << 30)
#define PACK_KEY_LUMA_MASK 0xffffffu    // the "has a coded level" bits that are luma and chroma contexts

// ---- the plan -----------------------------------------------------------------------------------------------------------------
extern "C" __global__ __launch_bounds__(256) void vp8_pack_key_plan_kernel(const uint8_t *coef, size_t coef_stride, uint8_t *scratch, PackLaunch L, PackKey K)
{
    __shared__ uint8_t s_end[8][32];
    constexpr int zz[16] = {0, 1, 4, 8, 5, 2, 3, 6, 9, 12, 13, 10, 7, 11, 14, 15};
    const int job = blockIdx.y, g = threadIdx.x >> 5, l = threadIdx.x & 31;
    const int nmb = L.mb_cols * L.mb_rows;
    const int mb = (int)blockIdx.x * 8 + g;
    const uint8_t *mode = K.modes + K.modes_stride * (size_t)job + (size_t)(mb < nmb ? mb : 0) * 32;
    const bool has_y2 = mode[0] != PACK_KEY_BPRED;
    const bool live = mb < nmb && l < (has_y2 ? 25 : 24);   // block 24 of a B_PRED macroblock is not read
    const int first = has_y2 && l < 16 ? 1 : 0;             // position 0 of a luma block: the Y2 block carries it where there is one
    int end = 0;
    bool bad = false;
    if (live) {
        const uint4 *b = (const uint4 *)(coef + coef_stride * (size_t)job + ((size_t)mb * 25 + l) * 32);
        const uint4 lo = b[0], hi = b[1];
        const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const int v = (int16_t)(w[zz[i] >> 1] >> (16 * (zz[i] & 1)));
            if (i >= first && v) {
                end = i + 1;
                bad |= v > PACK_MAX_LEVEL || v < -PACK_MAX_LEVEL;
            }
        }
    }
    s_end[g][l] = (uint8_t)end;
    const int half = (threadIdx.x >> 5) & 1;
    const uint32_t nz = (uint32_t)(__ballot(live && end > first) >> (32 * half)) & PACK_NZ_MASK;
    const bool any_bad = ((uint32_t)(__ballot(bad) >> (32 * half))) != 0;
    __syncthreads();
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
#pragma unroll
    for (int b = 0; b < 25; b++) rec[1 + b / 6] |= (uint32_t)s_end[g][b] << (5 * (b % 6));
    uint4 *out = (uint4 *)(pack_job(scratch, L, job) + (size_t)mb * PACK_RECORD_BYTES);
    out[0] = make_uint4(rec[0], rec[1], rec[2], rec[3]);
    out[1] = make_uint4(rec[4], rec[5], rec[6], rec[7]);
    uint32_t *ctr = pack_counters(scratch, job);
    if (status) atomicOr(&ctr[PACK_CTR_STATUS], status);
    if (!nz) atomicAdd(&ctr[PACK_CTR_SKIPPED], 1u);
    if (y == PACK_KEY_BPRED) atomicAdd(&ctr[PACK_CTR_MODES], 1u);
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
    const PackHead &H = L.heads[L.head_of[job]];
    uint8_t *area = pack_job(scratch, L, job);
    const int cols = L.mb_cols, nmb = L.mb_cols * L.mb_rows;
    PackCoder e;
    e.low = H.bottom; e.range = H.range; e.count = (int)H.bit_count;
    e.cache = H.cache; e.pending = H.pending;
    e.pos = 0; e.acc = 0;
    e.base = area + (size_t)nmb * PACK_RECORD_BYTES;
    e.cap = L.first_cap;
    const uint32_t settled = H.settled < PACK_HEAD_BYTES ? H.settled : PACK_HEAD_BYTES;
    for (uint32_t i = 0; i < settled; i++) pack_sink(e, H.bytes[i]);
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
    const uint32_t size = pack_finish(e);
    uint32_t *ctr = pack_counters(scratch, job);
    ctr[PACK_CTR_FIRST] = size;
    if (size > e.cap || size >= PACK_FIRST_LIMIT) atomicOr(&ctr[PACK_CTR_STATUS], PACK_OVERFLOW);
}

// ---- the token partitions -----------------------------------------------------------------------------------------------------
// A lane a token partition: vp8_pack_tokens_kernel with the default tables, except that a B_PRED macroblock has no Y2 block and
// codes its luma blocks as type 3 from step 0, and that the Y2 context is not the neighbouring macroblock's: above it is the
// record's bit (the y2 kernel's), to the left the lane carries it along its row past the B_PRED macroblocks.
extern "C" __global__ __launch_bounds__(PACK_CODER_THREADS) void vp8_pack_key_tokens_kernel(const uint8_t *coef, size_t coef_stride, uint8_t *scratch, int jobs,
                                                                                           PackLaunch L)
{
    __shared__ uint32_t s_coef[96 * PACK_ROW_BYTES / 4];
    __shared__ uint8_t s_cat[32];
    __shared__ uint4 s_block[PACK_CODER_THREADS][2];
    constexpr uint8_t cat_probs[26] = {159, 165, 145, 173, 148, 140, 176, 155, 140, 135, 180, 157, 141, 134, 130,
                                       254, 254, 243, 230, 196, 177, 153, 140, 133, 130, 129};
    for (int i = threadIdx.x; i < 96 * PACK_ROW_BYTES; i += PACK_CODER_THREADS) {
        const int row = i / PACK_ROW_BYTES, j = i - row * PACK_ROW_BYTES;
        ((uint8_t *)s_coef)[i] = j < 11 ? pack_tables::vp8t_default_coef_probs[row * 11 + j] : 0;
    }
    if (threadIdx.x < 26) s_cat[threadIdx.x] = cat_probs[threadIdx.x];
    __syncthreads();
    const int nparts = 1 << L.log2_parts;
    const int lane = (int)(blockIdx.x * PACK_CODER_THREADS + threadIdx.x);
    const int job = lane >> L.log2_parts, part = lane & (nparts - 1);
    if (job >= jobs) return;
    const int cols = L.mb_cols, nmb = L.mb_cols * L.mb_rows;
    uint8_t *area = pack_job(scratch, L, job);
    const uint4 *recs = (const uint4 *)area;
    const uint8_t *levels = coef + coef_stride * (size_t)job;
    typedef int16_t __attribute__((may_alias)) level_t;
    const level_t *mine = (const level_t *)s_block[threadIdx.x];
    PackCoder e;
    e.low = 0; e.range = 255; e.count = 24;
    e.cache = -1; e.pending = 0;
    e.pos = 0; e.acc = 0;
    e.base = area + (size_t)nmb * PACK_RECORD_BYTES + L.first_cap + (size_t)L.part_cap * part;
    e.cap = L.part_cap;
#pragma unroll 1
    for (int r = part; r < L.mb_rows; r += nparts) {
        uint32_t left = 0, left_y2 = 0;
#pragma unroll 1
        for (int c = 0; c < cols; c++) {
            const int mb = r * cols + c;
            const uint4 lo = recs[2 * mb];
            const uint32_t own = lo.x & PACK_NZ_MASK;
            const bool has_y2 = ((lo.x >> 25) & 7) != PACK_KEY_BPRED;
            if (!own) {                 // skipped: nothing is coded, its contexts are 0 -- the Y2 one only if it has a Y2 block
                left = 0;
                if (has_y2) left_y2 = 0;
                continue;
            }
            const uint32_t ew4 = recs[2 * mb + 1].x, ew5 = recs[2 * mb + 1].y;
            const uint32_t up = r ? recs[2 * (mb - cols)].x & PACK_KEY_LUMA_MASK : 0;
#pragma unroll 1
            for (int k = has_y2 ? 0 : 1; k < 25; k++) {     // Y2 where there is one, sixteen luma, four U, four V
                const int blk = k ? k - 1 : 24;
                const int type = k == 0 ? 1 : k <= 16 ? (has_y2 ? 0 : 3) : 2, first = has_y2 && k >= 1 && k <= 16;
                uint32_t a, l;
                if (blk == 24) {
                    a = lo.x >> 30; l = left_y2;
                } else if (blk < 16) {
                    a = blk >> 2 ? own >> (blk - 4) : up >> (blk + 12);
                    l = blk & 3 ? own >> (blk - 1) : left >> (blk + 3);
                } else {
                    const int q = (blk - 16) & 3;
                    a = q >> 1 ? own >> (blk - 2) : up >> (blk + 2);
                    l = q & 1 ? own >> (blk - 1) : left >> (blk + 1);
                }
                int ctx = (int)((a & 1) + (l & 1));
                const int word = blk / 6;
                const uint32_t ew = word == 0 ? lo.y : word == 1 ? lo.z : word == 2 ? lo.w : word == 3 ? ew4 : ew5;
                const int end = (int)(ew >> (5 * (blk - 6 * word))) & 31;
                if (end > first) {
                    const uint4 *b = (const uint4 *)(levels + ((size_t)mb * 25 + blk) * 32);
                    s_block[threadIdx.x][0] = b[0];
                    s_block[threadIdx.x][1] = b[1];
                }
                bool after_zero = false;
#pragma unroll 1
                for (int i = first; i < 16; i++) {
                    const int band = (int)(0x7666666665463210ull >> (4 * i)) & 15;
                    const uint32_t *p = s_coef + ((type * 8 + band) * 3 + ctx) * (PACK_ROW_BYTES / 4);
                    if (i >= end) {
                        pack_put(e, 0, p[0] & 0xffu);       // end of block
                        break;
                    }
                    const int v = mine[(0xfeb7adc963258410ull >> (4 * i)) & 15];
                    const int x = v < 0 ? -v : v;
                    if (!after_zero) pack_put(e, 1, PACK_P(0));
                    after_zero = x == 0;
                    if (x == 0) {
                        pack_put(e, 0, PACK_P(1));
                        ctx = 0;
                        continue;
                    }
                    pack_put(e, 1, PACK_P(1));
                    ctx = x == 1 ? 1 : 2;
                    if (x == 1) {
                        pack_put(e, 0, PACK_P(2));
                    } else {
                        pack_put(e, 1, PACK_P(2));
                        if (x <= 4) {
                            pack_put(e, 0, PACK_P(3));
                            pack_put(e, x != 2, PACK_P(4));
                            if (x != 2) pack_put(e, x - 3, PACK_P(5));
                        } else {
                            pack_put(e, 1, PACK_P(3));
                            const int cat = x < 7 ? 0 : x < 11 ? 1 : x < 19 ? 2 : x < 35 ? 3 : x < 67 ? 4 : 5;
                            pack_put(e, cat >= 2, PACK_P(6));
                            if (cat < 2) {
                                pack_put(e, cat, PACK_P(7));
                            } else {
                                pack_put(e, cat >= 4, PACK_P(8));
                                pack_put(e, cat & 1, cat < 4 ? PACK_P(9) : PACK_P(10));
                            }
                            const int bits = cat < 5 ? cat + 1 : 11, start = cat * (cat + 1) / 2;
                            const int extra = x - (cat < 5 ? 3 + (2 << cat) : 67);     // the categories begin at 5, 7, 11, 19, 35, 67
                            for (int j = 0; j < bits; j++) pack_put(e, (extra >> (bits - 1 - j)) & 1, s_cat[start + j]);
                        }
                    }
                    pack_put(e, v < 0, 128);
                }
            }
            left = own & PACK_KEY_LUMA_MASK;
            if (has_y2) left_y2 = own >> 24;
        }
    }
    const uint32_t size = pack_finish(e);
    uint32_t *ctr = pack_counters(scratch, job);
    ctr[PACK_CTR_PARTS + part] = size;
    if (size > e.cap) atomicOr(&ctr[PACK_CTR_STATUS], PACK_OVERFLOW);
}

// ---- the frame ----------------------------------------------------------------------------------------------------------------
// vp8_pack_assemble_kernel's job with the key frame's ten bytes in front: the tag with bit 0 clear, 9d 01 2a, width and height
extern "C" __global__ __launch_bounds__(256) void vp8_pack_key_assemble_kernel(const uint8_t *scratch, uint8_t *dst, size_t dst_stride, uint32_t *info,
                                                                              PackLaunch L, PackKey K)
{
    const int job = blockIdx.x, nparts = 1 << L.log2_parts;
    const uint32_t *ctr = (const uint32_t *)scratch + (size_t)job * PACK_CTR_DWORDS;
    const uint8_t *area = scratch + L.jobs_off + L.job_bytes * (size_t)job;
    const uint8_t *first_region = area + (size_t)L.mb_cols * L.mb_rows * PACK_RECORD_BYTES;
    uint8_t *out = dst + dst_stride * (size_t)job;
    const uint32_t first = ctr[PACK_CTR_FIRST];
    uint32_t status = ctr[PACK_CTR_STATUS];
    unsigned long long total = (unsigned long long)PACK_KEY_HEADER_BYTES + first + 3ull * (nparts - 1);
    for (int k = 0; k < nparts; k++) total += ctr[PACK_CTR_PARTS + k];
    if (total > L.cap) status |= PACK_OVERFLOW;
    const bool failed = status & (PACK_OVERFLOW | PACK_BAD_LEVEL | PACK_BAD_MODE);
    if (threadIdx.x == 0) {
        uint32_t *o = info + (size_t)job * 16;
        o[0] = status;
        o[1] = failed ? 0 : (uint32_t)total;
        o[2] = first;
        for (int k = 0; k < 8; k++) o[3 + k] = k < nparts ? ctr[PACK_CTR_PARTS + k] : 0;
        o[11] = ctr[PACK_CTR_SKIPPED];
        o[12] = ctr[PACK_CTR_MODES];    // B_PRED macroblocks
        o[13] = o[14] = o[15] = 0;
    }
    if (failed) return;
    if (threadIdx.x == 0) {
        const uint32_t tag = (uint32_t)L.version << 1 | (uint32_t)L.show_frame << 4 | first << 5;
        out[0] = (uint8_t)tag; out[1] = (uint8_t)(tag >> 8); out[2] = (uint8_t)(tag >> 16);
        out[3] = 0x9d; out[4] = 0x01; out[5] = 0x2a;
        out[6] = (uint8_t)K.width; out[7] = (uint8_t)((K.width >> 8) & 0x3f);
        out[8] = (uint8_t)K.height; out[9] = (uint8_t)((K.height >> 8) & 0x3f);
        for (int k = 0; k < nparts - 1; k++) {
            const uint32_t s = ctr[PACK_CTR_PARTS + k];
            uint8_t *t = out + PACK_KEY_HEADER_BYTES + first + 3 * k;
            t[0] = (uint8_t)s; t[1] = (uint8_t)(s >> 8); t[2] = (uint8_t)(s >> 16);
        }
    }
    for (uint32_t i = threadIdx.x; i < first; i += 256) out[PACK_KEY_HEADER_BYTES + i] = first_region[i];
    size_t at = PACK_KEY_HEADER_BYTES + (size_t)first + 3 * (size_t)(nparts - 1);
    for (int k = 0; k < nparts; k++) {
        const uint32_t s = ctr[PACK_CTR_PARTS + k];
        const uint8_t *region = first_region + L.first_cap + (size_t)L.part_cap * k;
        for (uint32_t i = threadIdx.x; i < s; i += 256) out[at + i] = region[i];
        at += s;
    }
}
