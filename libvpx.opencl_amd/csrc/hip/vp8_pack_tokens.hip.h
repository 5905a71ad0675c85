// Internal to libvp8hip.so: what the kernels of vp8_pack.hip, vp8_pack_adapt.hip and vp8_pack_key.hip share above the bool coder
// (vp8_pack_coder.hip.h), each piece once and every one __device__ __forceinline__: the scan order, the bands and the categories;
// a block's context and end out of a macroblock's record; the coder's two starts; the token coder of a block and the kernel of a
// token partition around it, a template over where the table comes from; the inter first-partition kernel, a template over ADAPT;
// the two halves the plan kernels have alike and the body of the assemble kernels.  The extern "C" kernels in the three files
// instantiate the templates under the names and argument lists the host launches; what differs by kind is `if constexpr`, so a
// kernel holds nothing of another kind's.
#pragma once
#include "vp8_pack_coder.hip.h"

#define PACK_KEY_BPRED 4
#define PACK_KEY_LUMA_MASK 0xffffffu    // the "has a coded level" bits that are luma and chroma contexts (key frames)

// step i of the scan: its position in the block (vp8_default_zig_zag1d) and its band (vp8_coef_bands), a nibble each
static __device__ __forceinline__ int pack_zigzag(int i) { return (int)(0xfeb7adc963258410ull >> (4 * i)) & 15; }
static __device__ __forceinline__ int pack_band(int i) { return (int)(0x7666666665463210ull >> (4 * i)) & 15; }
// DCT_CAT1..6 of a magnitude of 5 or more: the categories begin at 5, 7, 11, 19, 35, 67
static __device__ __forceinline__ int pack_category(int x) { return x < 7 ? 0 : x < 11 ? 1 : x < 19 ? 2 : x < 35 ? 3 : x < 67 ? 4 : 5; }

// The context of block blk: "the block above has a coded level" + "the block to the left has one", out of dword 0 of the records
// of the macroblock itself, of the one above and of the one to the left (0 for one outside the picture or skipped).  Block 24, the
// Y2 block, has the neighbours' Y2 blocks beside it: an inter frame's rule -- a key frame's token kernel has its own.
static __device__ __forceinline__ int pack_block_ctx(int blk, uint32_t own, uint32_t up, uint32_t left)
{
    uint32_t a, l;
    if (blk == 24) {
        a = up >> 24; l = left >> 24;
    } else if (blk < 16) {
        a = blk >> 2 ? own >> (blk - 4) : up >> (blk + 12);
        l = blk & 3 ? own >> (blk - 1) : left >> (blk + 3);
    } else {
        const int q = (blk - 16) & 3;
        a = q >> 1 ? own >> (blk - 2) : up >> (blk + 2);
        l = q & 1 ? own >> (blk - 1) : left >> (blk + 1);
    }
    return (int)((a & 1) + (l & 1));
}

// the end of block blk out of a record's five-bit fields: dwords 1..3 are lo's, 4 and 5 the next two
static __device__ __forceinline__ int pack_record_end(const uint4 &lo, uint32_t ew4, uint32_t ew5, int blk)
{
    const int word = blk / 6;
    const uint32_t ew = word == 0 ? lo.y : word == 1 ? lo.z : word == 2 ? lo.w : word == 3 ? ew4 : ew5;
    return (int)(ew >> (5 * (blk - 6 * word))) & 31;
}

// a coder at the start of a token partition, and one that goes on where the host's header ends
static __device__ __forceinline__ PackCoder pack_coder_fresh(uint8_t *base, uint32_t cap)
{
    PackCoder e;
    e.low = 0; e.range = 255; e.count = 24;
    e.cache = -1; e.pending = 0;
    e.pos = 0; e.acc = 0;
    e.base = base;
    e.cap = cap;
    return e;
}

static __device__ __forceinline__ PackCoder pack_coder_from_head(const PackHead &H, uint8_t *base, uint32_t cap)
{
    PackCoder e = pack_coder_fresh(base, cap);
    e.low = H.bottom; e.range = H.range; e.count = (int)H.bit_count;
    e.cache = H.cache; e.pending = H.pending;
    const uint32_t settled = H.settled < PACK_HEAD_BYTES ? H.settled : PACK_HEAD_BYTES;
    for (uint32_t i = 0; i < settled; i++) pack_sink(e, H.bytes[i]);
    return e;
}

// the end of a first-partition lane
static __device__ __forceinline__ void pack_first_done(PackCoder &e, uint8_t *scratch, int job)
{
    const uint32_t size = pack_finish(e);
    uint32_t *ctr = pack_counters(scratch, job);
    ctr[PACK_CTR_FIRST] = size;
    if (size > e.cap || size >= PACK_FIRST_LIMIT) atomicOr(&ctr[PACK_CTR_STATUS], PACK_OVERFLOW);
}

// the default coefficient table into LDS, a (type, band, context) row of 11 probabilities in PACK_ROW_BYTES
static __device__ __forceinline__ void pack_stage_default_rows(uint32_t *s_coef)
{
    for (int i = threadIdx.x; i < 96 * PACK_ROW_BYTES; i += PACK_CODER_THREADS) {
        const int row = i / PACK_ROW_BYTES, j = i - row * PACK_ROW_BYTES;
        ((uint8_t *)s_coef)[i] = j < 11 ? pack_tables::vp8t_default_coef_probs[row * 11 + j] : 0;
    }
}

// DCT_CAT1..6: the extra bits' probabilities back to back (RFC 6386 13.2); category cat starts at cat * (cat + 1) / 2
static __device__ __forceinline__ void pack_stage_cat_probs(uint8_t *s_cat)
{
    constexpr uint8_t cat_probs[26] = {159, 165, 145, 173, 148, 140, 176, 155, 140, 135, 180, 157, 141, 134, 130,
                                       254, 254, 243, 230, 196, 177, 153, 140, 133, 130, 129};
    if (threadIdx.x < 26) s_cat[threadIdx.x] = cat_probs[threadIdx.x];
}

// ---- the tokens of a block ----------------------------------------------------------------------------------------------------
typedef int16_t __attribute__((may_alias)) pack_level_t;    // (a lane's block, staged as two 16-byte pieces, read a level at a time)

// One block from step `first` to its end of block: per step the band's row of the lane's table (`table`: 96 rows of PACK_ROW_BYTES,
// (type, band, context)), the token tree, the extra bits and the sign (RFC 6386 13.2).  `mine`: the block's levels in LDS, read
// only below `end`; `ctx`: the context the neighbours give the first step.
static __device__ __forceinline__ void pack_block_tokens(PackCoder &e, const uint32_t *table, const uint8_t *s_cat, const pack_level_t *mine, int type,
                                                         int first, int end, int ctx)
{
    bool after_zero = false;
#pragma unroll 1
    for (int i = first; i < 16; i++) {
        const uint32_t *p = table + ((type * 8 + pack_band(i)) * 3 + ctx) * (PACK_ROW_BYTES / 4);
        if (i >= end) {
            pack_put(e, 0, p[0] & 0xffu);       // end of block
            break;
        }
        const int v = mine[pack_zigzag(i)];
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
                const int cat = pack_category(x);
                pack_put(e, cat >= 2, PACK_P(6));
                if (cat < 2) {
                    pack_put(e, cat, PACK_P(7));
                } else {
                    pack_put(e, cat >= 4, PACK_P(8));
                    pack_put(e, cat & 1, cat < 4 ? PACK_P(9) : PACK_P(10));
                }
                const int bits = cat < 5 ? cat + 1 : 11, start = cat * (cat + 1) / 2;
                const int extra = x - (cat < 5 ? 3 + (2 << cat) : 67);
                for (int j = 0; j < bits; j++) pack_put(e, (extra >> (bits - 1 - j)) & 1, s_cat[start + j]);
            }
        }
        pack_put(e, v < 0, 128);
    }
}

// ---- the token partitions -----------------------------------------------------------------------------------------------------
// A lane a token partition: the tokens of macroblock rows part, part + parts, ...  KIND says where the table comes from and what a
// macroblock is:
//   PACK_TOKENS_DEFAULT  inter frames, the default table, one copy in LDS.
//   PACK_TOKENS_OWN      inter frames, every job its own table: the lanes of a workgroup belong to 64 >> log2_parts jobs, and each
//                        job's effective table -- 96 rows of 12 bytes as the choose kernel left them in the job's adapt area -- has
//                        its own copy in LDS, 72 KB for 64 jobs; a lane reads a row of ITS job's copy with the same three-dword LDS
//                        load as the shared table's.
//   PACK_TOKENS_KEY      key frames, the default table.  A B_PRED macroblock has no Y2 block and codes its luma blocks as type 3
//                        from step 0, and the Y2 context is not the neighbouring macroblock's: above it is the record's bit 30
//                        (the y2 kernel's), to the left the lane carries it along its row past the B_PRED macroblocks.
enum { PACK_TOKENS_DEFAULT, PACK_TOKENS_OWN, PACK_TOKENS_KEY };

template <int KIND>
static __device__ __forceinline__ void pack_tokens(const uint8_t *coef, size_t coef_stride, uint8_t *scratch, int jobs, const PackLaunch &L,
                                                   [[maybe_unused]] const PackAdapt &A = {})
{
    constexpr bool KEY = KIND == PACK_TOKENS_KEY;
    constexpr uint32_t CTX_MASK = KEY ? PACK_KEY_LUMA_MASK : PACK_NZ_MASK;
    __shared__ uint32_t s_coef[(KIND == PACK_TOKENS_OWN ? PACK_CODER_THREADS : 1) * PACK_TABLE_DWORDS];
    __shared__ uint8_t s_cat[32];
    __shared__ uint4 s_block[PACK_CODER_THREADS][2];
    const uint32_t *table = s_coef;
    if constexpr (KIND == PACK_TOKENS_OWN) {
        const int per = PACK_CODER_THREADS >> L.log2_parts;     // jobs of a workgroup
#pragma unroll 1
        for (int i = threadIdx.x; i < per * PACK_TABLE_DWORDS; i += PACK_CODER_THREADS) {
            const int slot = i / PACK_TABLE_DWORDS, j = (int)blockIdx.x * per + slot;
            s_coef[i] = j < jobs ? ((const uint32_t *)(pack_adapt_job(scratch, A, j) + PACK_ADAPT_ROWS))[i - slot * PACK_TABLE_DWORDS] : 0u;
        }
        table = s_coef + (threadIdx.x >> L.log2_parts) * PACK_TABLE_DWORDS;
    } else {
        pack_stage_default_rows(s_coef);
    }
    pack_stage_cat_probs(s_cat);
    __syncthreads();
    const int nparts = 1 << L.log2_parts;
    const int lane = (int)(blockIdx.x * PACK_CODER_THREADS + threadIdx.x);
    const int job = lane >> L.log2_parts, part = lane & (nparts - 1);
    if (job >= jobs) return;
    const int cols = L.mb_cols, nmb = L.mb_cols * L.mb_rows;
    uint8_t *area = pack_job(scratch, L, job);
    const uint4 *recs = (const uint4 *)area;
    const uint8_t *levels = coef + coef_stride * (size_t)job;
    const pack_level_t *mine = (const pack_level_t *)s_block[threadIdx.x];
    PackCoder e = pack_coder_fresh(area + (size_t)nmb * PACK_RECORD_BYTES + L.first_cap + (size_t)L.part_cap * part, L.part_cap);
#pragma unroll 1
    for (int r = part; r < L.mb_rows; r += nparts) {
        uint32_t left = 0;
        [[maybe_unused]] uint32_t left_y2 = 0;
#pragma unroll 1
        for (int c = 0; c < cols; c++) {
            const int mb = r * cols + c;
            const uint4 lo = recs[2 * mb];
            const uint32_t own = lo.x & PACK_NZ_MASK;
            bool has_y2 = true;
            if constexpr (KEY) has_y2 = ((lo.x >> 25) & 7) != PACK_KEY_BPRED;
            if (!own) {                 // skipped: nothing is coded, its contexts are 0 -- the Y2 one only if it has a Y2 block
                left = 0;
                if constexpr (KEY)
                    if (has_y2) left_y2 = 0;
                continue;
            }
            const uint32_t ew4 = recs[2 * mb + 1].x, ew5 = recs[2 * mb + 1].y;
            const uint32_t up = r ? recs[2 * (mb - cols)].x & CTX_MASK : 0;
#pragma unroll 1
            for (int k = has_y2 ? 0 : 1; k < 25; k++) {     // Y2 where there is one, sixteen luma, four U, four V
                const int blk = k ? k - 1 : 24;
                const int type = k == 0 ? 1 : k <= 16 ? (has_y2 ? 0 : 3) : 2, first = has_y2 && k >= 1 && k <= 16;
                int ctx = pack_block_ctx(blk, own, up, left);
                if constexpr (KEY)
                    if (blk == 24) ctx = (int)(((lo.x >> 30) & 1) + (left_y2 & 1));
                const int end = pack_record_end(lo, ew4, ew5, blk);
                if (end > first) {
                    const uint4 *b = (const uint4 *)(levels + ((size_t)mb * 25 + blk) * 32);
                    s_block[threadIdx.x][0] = b[0];
                    s_block[threadIdx.x][1] = b[1];
                }
                pack_block_tokens(e, table, s_cat, mine, type, first, end, ctx);
            }
            left = own & CTX_MASK;
            if constexpr (KEY)
                if (has_y2) left_y2 = own >> 24;
        }
    }
    const uint32_t size = pack_finish(e);
    uint32_t *ctr = pack_counters(scratch, job);
    ctr[PACK_CTR_PARTS + part] = size;
    if (size > e.cap) atomicOr(&ctr[PACK_CTR_STATUS], PACK_OVERFLOW);
}

// ---- the first partition of an inter frame ----------------------------------------------------------------------------------------
// A lane a job, behind the header the host coded.  ADAPT: the host's header ends behind refresh_last; the lane codes the rest of it
// from what the choose kernel left in the job's adapt area -- per probability the update flag and the effective value; the four
// header probabilities --, then the macroblocks with the job's effective vector probabilities and prob_skip_false, each lane's in
// its own 40 bytes of LDS.
template <bool ADAPT>
static __device__ __forceinline__ void pack_first(uint8_t *scratch, int jobs, const PackLaunch &L, [[maybe_unused]] const PackAdapt &A = {})
{
    __shared__ uint32_t s_mvcs[(ADAPT ? PACK_CODER_THREADS : 1) * 10];      // (40 bytes: the 38 and two of the reserved)
    const uint8_t *s_mvc = (const uint8_t *)s_mvcs;
    if constexpr (ADAPT) {
        if ((int)(blockIdx.x * PACK_CODER_THREADS + threadIdx.x) < jobs) {
            const uint32_t *set = (const uint32_t *)(pack_adapt_job(scratch, A, (int)(blockIdx.x * PACK_CODER_THREADS + threadIdx.x)) + PACK_ADAPT_EFF + 1056);
            for (int i = 0; i < 10; i++) s_mvcs[threadIdx.x * 10 + i] = set[i];
        }
        s_mvc = (const uint8_t *)(s_mvcs + threadIdx.x * 10);
    } else {
        if (threadIdx.x < 38) ((uint8_t *)s_mvcs)[threadIdx.x] = pack_tables::vp8t_default_mv_context[threadIdx.x];
    }
    __syncthreads();
    const int job = (int)(blockIdx.x * PACK_CODER_THREADS + threadIdx.x);
    if (job >= jobs) return;
    uint8_t *area = pack_job(scratch, L, job);
    const int nmb = L.mb_cols * L.mb_rows;
    PackCoder e = pack_coder_from_head(L.heads[L.head_of[job]], area + (size_t)nmb * PACK_RECORD_BYTES, L.first_cap);
    uint32_t prob_skip = (uint32_t)L.prob_skip, prob_intra = (uint32_t)L.prob_intra, prob_last = (uint32_t)L.prob_last, prob_gf = (uint32_t)L.prob_gf;
    if constexpr (ADAPT) {
        // The probability section, one item after the other through ONE put: 1056 coefficient items -- the flag at
        // vp8_coef_update_probs, then the new value in 8 bits where it is set --, five items without a flag -- mb_no_coeff_skip (1),
        // prob_skip_false, prob_intra, prob_last, prob_gf with the two intra update flags (0) behind it -- and 38 vector items -- the
        // flag at vp8_mv_update_probs, then the new value >> 1 in 7 bits.
        const uint8_t *ad = pack_adapt_job(scratch, A, job);
        const uint8_t *eff = ad + PACK_ADAPT_EFF, *flag = ad + PACK_ADAPT_FLAG;
        const uint32_t *hdr = (const uint32_t *)(ad + PACK_ADAPT_HDR);
        prob_skip = hdr[PACK_ADAPT_HDR_SKIP]; prob_intra = hdr[PACK_ADAPT_HDR_INTRA]; prob_last = hdr[PACK_ADAPT_HDR_LAST]; prob_gf = hdr[PACK_ADAPT_HDR_GF];
#pragma unroll 1
        for (int item = 0; item < 1056 + 5 + 38; item++) {
            uint32_t value, fprob = 0;
            int bits, u = 1, j = 0;         // j: -1 the flag, then the literal's bits
            if (item < 1056) {
                value = eff[item]; bits = 8; u = flag[item] & 1; fprob = pack_tables::vp8t_coef_update_probs[item]; j = -1;
            } else if (item < 1056 + 5) {
                const int k = item - 1056;
                value = k == 0 ? 1u : k == 1 ? prob_skip : k == 2 ? prob_intra : k == 3 ? prob_last : prob_gf << 2;
                bits = k == 0 ? 1 : k == 4 ? 10 : 8;
            } else {
                const int k = item - 1056 - 5;
                value = (uint32_t)s_mvc[k] >> 1; bits = 7; u = flag[1056 + k] & 1; fprob = pack_tables::vp8t_mv_update_probs[k]; j = -1;
            }
            if (!u) bits = 0;
#pragma unroll 1
            for (; j < bits; j++) pack_put(e, j < 0 ? u : (int)(value >> (bits - 1 - j)) & 1, j < 0 ? fprob : 128u);
        }
    }
    const uint4 *recs = (const uint4 *)area;
#pragma unroll 1
    for (int mb = 0; mb < nmb; mb++) {
        const uint32_t w0 = recs[2 * mb].x;
        const uint4 hi = recs[2 * mb + 1];
        const int mode = (int)(w0 >> 25) & 3;
        pack_put(e, !(w0 & PACK_NZ_MASK), prob_skip);
        pack_put(e, 1, prob_intra);
        pack_put(e, L.ref_frame != 1, prob_last);
        if (L.ref_frame != 1) pack_put(e, L.ref_frame - 2, prob_gf);
        pack_put(e, mode != 0, hi.z & 0xff);
        if (mode != 0) {
            pack_put(e, mode != 1, (hi.z >> 8) & 0xff);
            if (mode != 1) {
                pack_put(e, mode != 2, (hi.z >> 16) & 0xff);
                if (mode != 2) {
                    pack_put(e, 0, hi.z >> 24);
                    pack_mv_component(e, (int16_t)(hi.w & 0xffff), s_mvc);
                    pack_mv_component(e, (int16_t)(hi.w >> 16), s_mvc + 19);
                }
            }
        }
    }
    pack_first_done(e, scratch, job);
}

// ---- the plan kernels' two halves -------------------------------------------------------------------------------------------------
// A lane a block, 32 lanes a macroblock (l = threadIdx.x & 31, eight macroblocks a workgroup of 256): block l of macroblock mb of
// the job's `levels`, where `live`, gives its end -- 1 + the last step from `first` on that has a level, 0 for none -- into ends[l]
// and whether a level is out of range; the macroblock's lanes get nz, "block b has a coded level", and any_bad.  The workgroup
// meets behind it: every lane comes here.
static __device__ __forceinline__ void pack_plan_scan(const uint8_t *levels, int mb, int first, bool live, uint8_t *ends, uint32_t &nz, bool &any_bad)
{
    const int l = threadIdx.x & 31;
    int end = 0;
    bool bad = false;
    if (live) {
        const uint4 *b = (const uint4 *)(levels + ((size_t)mb * 25 + l) * 32);
        const uint4 lo = b[0], hi = b[1];
        const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const int z = pack_zigzag(i), v = (int16_t)(w[z >> 1] >> (16 * (z & 1)));
            if (i >= first && v) {
                end = i + 1;
                bad |= v > PACK_MAX_LEVEL || v < -PACK_MAX_LEVEL;
            }
        }
    }
    ends[l] = (uint8_t)end;
    const int half = (threadIdx.x >> 5) & 1;
    nz = (uint32_t)(__ballot(live && end > first) >> (32 * half)) & PACK_NZ_MASK;
    any_bad = ((uint32_t)(__ballot(bad) >> (32 * half))) != 0;
    __syncthreads();
}

// A macroblock's first lane leaves the record: rec[0] with nz in its low bits, rec[6..7] the kernel's own, dwords 1..5 (given as
// 0) the blocks' ends; then the job's status bits and skipped count.
static __device__ __forceinline__ void pack_record_store(uint8_t *scratch, const PackLaunch &L, int job, int mb, uint32_t (&rec)[8], const uint8_t *ends,
                                                         uint32_t status)
{
#pragma unroll
    for (int b = 0; b < 25; b++) rec[1 + b / 6] |= (uint32_t)ends[b] << (5 * (b % 6));
    uint4 *out = (uint4 *)(pack_job(scratch, L, job) + (size_t)mb * PACK_RECORD_BYTES);
    out[0] = make_uint4(rec[0], rec[1], rec[2], rec[3]);
    out[1] = make_uint4(rec[4], rec[5], rec[6], rec[7]);
    uint32_t *ctr = pack_counters(scratch, job);
    if (status) atomicOr(&ctr[PACK_CTR_STATUS], status);
    if (!(rec[0] & PACK_NZ_MASK)) atomicAdd(&ctr[PACK_CTR_SKIPPED], 1u);
}

// ---- the frame ----------------------------------------------------------------------------------------------------------------
// A workgroup of 256 a job: the job's info; then, unless a bit of `fatal` is set, HEADER bytes, the first partition, the size table
// and the token partitions into the job's dst.  What the kernels do not share they hand in, both run by lane 0:
// info_tail(o, ctr) writes o[12..15] from the job's counters, head(out, first) the HEADER bytes in front of the frame.
template <int HEADER, class InfoTail, class Head>
static __device__ __forceinline__ void pack_assemble(const uint8_t *scratch, uint8_t *dst, size_t dst_stride, uint32_t *info, const PackLaunch &L,
                                                     uint32_t fatal, InfoTail info_tail, Head head)
{
    const int job = blockIdx.x, nparts = 1 << L.log2_parts;
    const uint32_t *ctr = (const uint32_t *)scratch + (size_t)job * PACK_CTR_DWORDS;
    const uint8_t *area = scratch + L.jobs_off + L.job_bytes * (size_t)job;
    const uint8_t *first_region = area + (size_t)L.mb_cols * L.mb_rows * PACK_RECORD_BYTES;
    uint8_t *out = dst + dst_stride * (size_t)job;
    const uint32_t first = ctr[PACK_CTR_FIRST];
    uint32_t status = ctr[PACK_CTR_STATUS];
    unsigned long long total = (unsigned long long)HEADER + first + 3ull * (nparts - 1);
    for (int k = 0; k < nparts; k++) total += ctr[PACK_CTR_PARTS + k];
    if (total > L.cap) status |= PACK_OVERFLOW;
    const bool failed = status & fatal;
    if (threadIdx.x == 0) {
        uint32_t *o = info + (size_t)job * 16;
        o[0] = status;
        o[1] = failed ? 0 : (uint32_t)total;
        o[2] = first;
        for (int k = 0; k < 8; k++) o[3 + k] = k < nparts ? ctr[PACK_CTR_PARTS + k] : 0;
        o[11] = ctr[PACK_CTR_SKIPPED];
        info_tail(o, ctr);
    }
    if (failed) return;
    if (threadIdx.x == 0) {
        head(out, first);
        for (int k = 0; k < nparts - 1; k++) {
            const uint32_t s = ctr[PACK_CTR_PARTS + k];
            uint8_t *t = out + HEADER + first + 3 * k;
            t[0] = (uint8_t)s; t[1] = (uint8_t)(s >> 8); t[2] = (uint8_t)(s >> 16);
        }
    }
    for (uint32_t i = threadIdx.x; i < first; i += 256) out[HEADER + i] = first_region[i];
    size_t at = HEADER + (size_t)first + 3 * (size_t)(nparts - 1);
    for (int k = 0; k < nparts; k++) {
        const uint32_t s = ctr[PACK_CTR_PARTS + k];
        const uint8_t *region = first_region + L.first_cap + (size_t)L.part_cap * k;
        for (uint32_t i = threadIdx.x; i < s; i += 256) out[at + i] = region[i];
        at += s;
    }
}
