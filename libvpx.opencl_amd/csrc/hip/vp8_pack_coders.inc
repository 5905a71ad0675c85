// The two coder kernels of the frame packer, included once by vp8_pack.hip (PACK_ADAPT 0: vp8_pack_first_kernel,
// vp8_pack_tokens_kernel -- the default tables, the header complete from the host) and once by vp8_pack_adapt.hip (PACK_ADAPT 1:
// vp8_pack_first_adapt_kernel, vp8_pack_tokens_adapt_kernel -- every job its own tables, the header's probability section coded
// here).  With PACK_ADAPT 0 the text is what vp8_pack.hip held.
#if PACK_ADAPT
#define PACK_KERNEL(name) name##_adapt_kernel
#define PACK_ADAPT_ARG , PackAdapt A
#define PACK_PROB(x) prob_##x
#define PACK_TABLE table
#else
#define PACK_KERNEL(name) name##_kernel
#define PACK_ADAPT_ARG
#define PACK_PROB(x) (uint32_t)L.prob_##x
#define PACK_TABLE s_coef
#endif

// ---- the first partition ------------------------------------------------------------------------------------------------------
// A lane a job.  PACK_ADAPT: the host's header ends behind refresh_last; the lane codes the rest of it from what the choose kernel
// left in the job's adapt area -- per probability the update flag and the effective value; the four header probabilities --, then
// the macroblocks with the job's effective vector probabilities and prob_skip_false, each lane's in its own 40 bytes of LDS.
extern "C" __global__ __launch_bounds__(PACK_CODER_THREADS) void PACK_KERNEL(vp8_pack_first)(uint8_t *scratch, int jobs, PackLaunch L PACK_ADAPT_ARG)
{
#if PACK_ADAPT
    __shared__ uint32_t s_mvcs[PACK_CODER_THREADS * 10];
    if ((int)(blockIdx.x * PACK_CODER_THREADS + threadIdx.x) < jobs) {
        const uint32_t *set = (const uint32_t *)(pack_adapt_job(scratch, A, (int)(blockIdx.x * PACK_CODER_THREADS + threadIdx.x)) + PACK_ADAPT_EFF + 1056);
        for (int i = 0; i < 10; i++) s_mvcs[threadIdx.x * 10 + i] = set[i];     // (40 bytes: the 38 and two of the reserved)
    }
    const uint8_t *s_mvc = (const uint8_t *)(s_mvcs + threadIdx.x * 10);
#else
    __shared__ uint8_t s_mvc[40];
    if (threadIdx.x < 38) s_mvc[threadIdx.x] = pack_tables::vp8t_default_mv_context[threadIdx.x];
#endif
    __syncthreads();
    const int job = (int)(blockIdx.x * PACK_CODER_THREADS + threadIdx.x);
    if (job >= jobs) return;
    const PackHead &H = L.heads[L.head_of[job]];
    uint8_t *area = pack_job(scratch, L, job);
    const int nmb = L.mb_cols * L.mb_rows;
    PackCoder e;
    e.low = H.bottom; e.range = H.range; e.count = (int)H.bit_count;
    e.cache = H.cache; e.pending = H.pending;
    e.pos = 0; e.acc = 0;
    e.base = area + (size_t)nmb * PACK_RECORD_BYTES;
    e.cap = L.first_cap;
    const uint32_t settled = H.settled < PACK_HEAD_BYTES ? H.settled : PACK_HEAD_BYTES;
    for (uint32_t i = 0; i < settled; i++) pack_sink(e, H.bytes[i]);
#if PACK_ADAPT
    // The probability section, one item after the other through ONE put: 1056 coefficient items -- the flag at
    // vp8_coef_update_probs, then the new value in 8 bits where it is set --, five items without a flag -- mb_no_coeff_skip (1),
    // prob_skip_false, prob_intra, prob_last, prob_gf with the two intra update flags (0) behind it -- and 38 vector items -- the
    // flag at vp8_mv_update_probs, then the new value >> 1 in 7 bits.
    const uint8_t *ad = pack_adapt_job(scratch, A, job);
    const uint8_t *eff = ad + PACK_ADAPT_EFF, *flag = ad + PACK_ADAPT_FLAG;
    const uint32_t *hdr = (const uint32_t *)(ad + PACK_ADAPT_HDR);
    const uint32_t prob_skip = hdr[PACK_ADAPT_HDR_SKIP], prob_intra = hdr[PACK_ADAPT_HDR_INTRA], prob_last = hdr[PACK_ADAPT_HDR_LAST],
                   prob_gf = hdr[PACK_ADAPT_HDR_GF];
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
#endif
    const uint4 *recs = (const uint4 *)area;
#pragma unroll 1
    for (int mb = 0; mb < nmb; mb++) {
        const uint32_t w0 = recs[2 * mb].x;
        const uint4 hi = recs[2 * mb + 1];
        const int mode = (int)(w0 >> 25) & 3;
        pack_put(e, !(w0 & PACK_NZ_MASK), PACK_PROB(skip));
        pack_put(e, 1, PACK_PROB(intra));
        pack_put(e, L.ref_frame != 1, PACK_PROB(last));
        if (L.ref_frame != 1) pack_put(e, L.ref_frame - 2, PACK_PROB(gf));
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
    const uint32_t size = pack_finish(e);
    uint32_t *ctr = pack_counters(scratch, job);
    ctr[PACK_CTR_FIRST] = size;
    if (size > e.cap || size >= PACK_FIRST_LIMIT) atomicOr(&ctr[PACK_CTR_STATUS], PACK_OVERFLOW);
}

// ---- the token partitions -----------------------------------------------------------------------------------------------------
// A lane a token partition.  PACK_ADAPT: the lanes of a workgroup belong to 64 >> log2_parts jobs, and each job's effective table
// -- 96 rows of 12 bytes as the choose kernel left them in the job's adapt area -- has its own copy in LDS, 72 KB for 64 jobs; a
// lane reads a row of ITS job's copy with the same three-dword LDS load as the shared table's.
extern "C" __global__ __launch_bounds__(PACK_CODER_THREADS) void PACK_KERNEL(vp8_pack_tokens)(const uint8_t *coef, size_t coef_stride, uint8_t *scratch,
                                                                                             int jobs, PackLaunch L PACK_ADAPT_ARG)
{
#if PACK_ADAPT
    __shared__ uint32_t s_coef[PACK_CODER_THREADS * PACK_TABLE_DWORDS];
#else
    __shared__ uint32_t s_coef[96 * PACK_ROW_BYTES / 4];
#endif
    __shared__ uint8_t s_cat[32];
    __shared__ uint4 s_block[PACK_CODER_THREADS][2];
    // DCT_CAT1..6: the extra bits' probabilities back to back (RFC 6386 13.2); a category's start and length
    constexpr uint8_t cat_probs[26] = {159, 165, 145, 173, 148, 140, 176, 155, 140, 135, 180, 157, 141, 134, 130,
                                       254, 254, 243, 230, 196, 177, 153, 140, 133, 130, 129};
#if PACK_ADAPT
    const int per = PACK_CODER_THREADS >> L.log2_parts;     // jobs of a workgroup
#pragma unroll 1
    for (int i = threadIdx.x; i < per * PACK_TABLE_DWORDS; i += PACK_CODER_THREADS) {
        const int slot = i / PACK_TABLE_DWORDS, j = (int)blockIdx.x * per + slot;
        s_coef[i] = j < jobs ? ((const uint32_t *)(pack_adapt_job(scratch, A, j) + PACK_ADAPT_ROWS))[i - slot * PACK_TABLE_DWORDS] : 0u;
    }
    const uint32_t *table = s_coef + (threadIdx.x >> L.log2_parts) * PACK_TABLE_DWORDS;
#else
    for (int i = threadIdx.x; i < 96 * PACK_ROW_BYTES; i += PACK_CODER_THREADS) {
        const int row = i / PACK_ROW_BYTES, j = i - row * PACK_ROW_BYTES;
        ((uint8_t *)s_coef)[i] = j < 11 ? pack_tables::vp8t_default_coef_probs[row * 11 + j] : 0;
    }
#endif
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
    typedef int16_t __attribute__((may_alias)) level_t;     // (the lane's block, staged as two 16-byte pieces, read a level at a time)
    const level_t *mine = (const level_t *)s_block[threadIdx.x];
    PackCoder e;
    e.low = 0; e.range = 255; e.count = 24;
    e.cache = -1; e.pending = 0;
    e.pos = 0; e.acc = 0;
    e.base = area + (size_t)nmb * PACK_RECORD_BYTES + L.first_cap + (size_t)L.part_cap * part;
    e.cap = L.part_cap;
#pragma unroll 1
    for (int r = part; r < L.mb_rows; r += nparts) {
        uint32_t left = 0;
#pragma unroll 1
        for (int c = 0; c < cols; c++) {
            const int mb = r * cols + c;
            const uint4 lo = recs[2 * mb];
            const uint32_t own = lo.x & PACK_NZ_MASK;
            if (!own) {                 // skipped: nothing is coded and its contexts are 0
                left = 0;
                continue;
            }
            const uint32_t ew4 = recs[2 * mb + 1].x, ew5 = recs[2 * mb + 1].y;
            const uint32_t up = r ? recs[2 * (mb - cols)].x & PACK_NZ_MASK : 0;
#pragma unroll 1
            for (int k = 0; k < 25; k++) {                  // Y2, sixteen luma, four U, four V
                const int blk = k ? k - 1 : 24;
                const int type = k == 0 ? 1 : k <= 16 ? 0 : 2, first = k >= 1 && k <= 16;
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
                    const uint32_t *p = PACK_TABLE + ((type * 8 + band) * 3 + ctx) * (PACK_ROW_BYTES / 4);
                    if (i >= end) {
                        pack_put(e, 0, p[0] & 0xffu);       // end of block
                        break;
                    }
                    const int v = mine[(0xfeb7adc963258410ull >> (4 * i)) & 15];
                    const int x = v < 0 ? -v : v;
                    // the token tree and the extra bits (RFC 6386 13.2), one coefficient
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
            left = own;
        }
    }
    const uint32_t size = pack_finish(e);
    uint32_t *ctr = pack_counters(scratch, job);
    ctr[PACK_CTR_PARTS + part] = size;
    if (size > e.cap) atomicOr(&ctr[PACK_CTR_STATUS], PACK_OVERFLOW);
}

#undef PACK_KERNEL
#undef PACK_ADAPT_ARG
#undef PACK_PROB
#undef PACK_TABLE
