// The kernels of vp8hip_frames_pack_async (include/vp8hip.h has the definition, vp8hip_pack.hip the plan): compressed VP8 inter
// frames from frames_quant's levels and vectors.
//   vp8_pack_plan_kernel      parallel: a lane a block finds the block's end and checks its levels; a lane a macroblock finds the
//                             skip flag, the mode among ZEROMV / NEARESTMV / NEARMV / NEWMV, the coded difference and the vector
//                             checks, and leaves the macroblock's record (vp8_pack.hip.h) in the scratch.
//   vp8_pack_first_kernel     a lane a job: the first partition behind the header the host coded (vp8hip_pack_header).
//   vp8_pack_tokens_kernel    a lane a token partition: the tokens of macroblock rows part, part + parts, ...
//   vp8_pack_assemble_kernel  a workgroup a job: tag, partitions and size table into the caller's memory, the job's info.
// The two coder kernels are launches of their own because their lanes do very different amounts of work and the lanes of a wave go
// through their loops together.  The bool coder is RFC 6386 section 7.3 with the carry deferred: the last byte that is not 0xFF
// is held back (cache) with the count of 0xFF bytes behind it (pending), so a carry never walks back through stored bytes, and
// settled bytes leave in whole dwords.  Every store is checked against the end of the lane's region; a lane whose region is full
// goes on counting.
#include <hip/hip_runtime.h>
#include "vp8_pack.hip.h"

#define PACK_CODER_THREADS 64
#define PACK_ROW_BYTES 12               // a (type, band, context) row of 11 probabilities in LDS, read as three dwords

struct PackCoder {
    uint32_t low, range;
    int count;                          // shifts until the next byte is complete
    int cache;                          // -1: none yet
    uint32_t pending;
    uint32_t pos, acc;                  // bytes that have left; those of them that wait for their dword
    uint8_t *base;
    uint32_t cap;
};

static __device__ __forceinline__ void pack_sink(PackCoder &e, uint32_t byte)
{
    e.acc |= (byte & 0xffu) << (8 * (e.pos & 3));
    e.pos++;
    if (!(e.pos & 3)) {
        if (e.pos <= e.cap) *(uint32_t *)(e.base + e.pos - 4) = e.acc;
        e.acc = 0;
    }
}

// a complete byte, bit 8 the carry into what came before it
static __device__ __forceinline__ void pack_emit(PackCoder &e, uint32_t b)
{
    if (b & 0x100u) {
        pack_sink(e, (uint32_t)e.cache + 1);
        for (; e.pending; e.pending--) pack_sink(e, 0);
        e.cache = (int)(b & 0xffu);
    } else if (b == 0xffu && e.cache >= 0) {
        e.pending++;
    } else {
        if (e.cache >= 0) pack_sink(e, (uint32_t)e.cache);
        for (; e.pending; e.pending--) pack_sink(e, 0xffu);
        e.cache = (int)b;
    }
}

static __device__ __forceinline__ void pack_put(PackCoder &e, int bit, uint32_t prob)
{
    const uint32_t split = 1 + (((e.range - 1) * prob) >> 8);
    if (bit) {
        e.low += split;
        e.range -= split;
    } else {
        e.range = split;
    }
    int s = __clz((int)e.range) - 24;   // range is 1..255: 0..7 shifts bring it back to 128..255
    e.range <<= s;
    if (s >= e.count) {
        const int c = e.count;          // the byte is bits 24 - c .. 31 - c of low, the carry the bit above
        pack_emit(e, e.low >> (24 - c));
        e.low = (e.low & ((1u << (24 - c)) - 1)) << c;
        s -= c;
        e.count = 8;
    }
    e.low <<= s;
    e.count -= s;
}

// BoolEncoder.finish: the rest of the byte in the making and three more; then what was held back.  Returns the partition's bytes.
static __device__ uint32_t pack_finish(PackCoder &e)
{
    const int c = e.count;
    pack_emit(e, e.low >> (24 - c));
    const uint32_t rest = (e.low & ((1u << (24 - c)) - 1)) << c;
    pack_emit(e, (rest >> 16) & 0xffu);
    pack_emit(e, (rest >> 8) & 0xffu);
    pack_emit(e, rest & 0xffu);
    if (e.cache >= 0) pack_sink(e, (uint32_t)e.cache);
    for (; e.pending; e.pending--) pack_sink(e, 0xffu);
    if ((e.pos & 3) && ((e.pos + 3) & ~3u) <= e.cap) *(uint32_t *)(e.base + (e.pos & ~3u)) = e.acc;
    return e.pos;
}

static __device__ __forceinline__ uint32_t *pack_counters(uint8_t *scratch, int job) { return (uint32_t *)scratch + (size_t)job * PACK_CTR_DWORDS; }
static __device__ __forceinline__ uint8_t *pack_job(uint8_t *scratch, const PackLaunch &L, int job) { return scratch + L.jobs_off + L.job_bytes * (size_t)job; }

// ---- the plan -----------------------------------------------------------------------------------------------------------------
struct PackMv { int r, c; };
static __device__ __forceinline__ bool pack_same(PackMv a, PackMv b) { return a.r == b.r && a.c == b.c; }
static __device__ __forceinline__ int pack_clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

extern "C" __global__ __launch_bounds__(256) void vp8_pack_plan_kernel(const uint8_t *mv, size_t mv_stride, const uint8_t *coef, size_t coef_stride,
                                                                       uint8_t *scratch, PackLaunch L)
{
    __shared__ uint8_t s_end[8][32];
    constexpr int zz[16] = {0, 1, 4, 8, 5, 2, 3, 6, 9, 12, 13, 10, 7, 11, 14, 15};
    const int job = blockIdx.y, g = threadIdx.x >> 5, l = threadIdx.x & 31;
    const int cols = L.mb_cols, nmb = L.mb_cols * L.mb_rows;
    const int mb = (int)blockIdx.x * 8 + g;
    const bool live = mb < nmb && l < 25;
    const int first = l < 16 ? 1 : 0;   // position 0 of a luma block is not coded: the Y2 block carries it
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

    const int r = mb / cols, c = mb - r * cols;
    const int16_t *m = (const int16_t *)(mv + mv_stride * (size_t)job);
    auto vec = [&](int rr, int cc) {
        PackMv v = {0, 0};
        if (L.has_mv) { v.c = m[rr * cols + cc]; v.r = m[nmb + rr * cols + cc]; }
        return v;
    };
    const PackMv v = vec(r, c);
    uint32_t status = ((v.r | v.c) & 1) ? PACK_BAD_VECTOR : 0;
    if (any_bad) status |= PACK_BAD_LEVEL;
    // vp8_find_near_mvs (RFC 6386 18.3) over above, left, above-left; every neighbour inside the picture is an inter macroblock of
    // the same reference frame with the given vector, one outside counts as intra
    PackMv near[4] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}};
    int cnt[4] = {0, 0, 0, 0}, k = 0;
    for (int n = 0; n < 3; n++) {
        const int rr = n == 1 ? r : r - 1, cc = n == 0 ? c : c - 1, weight = n == 2 ? 1 : 2;
        if (rr < 0 || cc < 0) continue;
        const PackMv t = vec(rr, cc);
        if (t.r | t.c) {
            if (k == 0 || !pack_same(t, near[k])) near[++k] = t;
            cnt[k] += weight;
        } else {
            cnt[0] += weight;
        }
    }
    const int left = -((c * 16) << 3), right = ((cols - 1 - c) * 16) << 3, top = -((r * 16) << 3), bottom = ((L.mb_rows - 1 - r) * 16) << 3;
    auto clamped = [&](PackMv t) { return PackMv{pack_clampi(t.r, top - 128, bottom + 128), pack_clampi(t.c, left - 128, right + 128)}; };
    const int32_t *mc = pack_tables::vp8t_mode_contexts;
    uint32_t probs = (uint32_t)mc[cnt[0] * 4];
    int mode = 0, dr = 0, dc = 0;
    if (v.r | v.c) {
        if (cnt[3] && pack_same(near[k], near[1])) cnt[1]++;
        if (cnt[2] > cnt[1]) {
            const int t = cnt[1]; cnt[1] = cnt[2]; cnt[2] = t;
            const PackMv s = near[1]; near[1] = near[2]; near[2] = s;
        }
        probs |= (uint32_t)mc[cnt[1] * 4 + 1] << 8;
        mode = 1;
        if (!pack_same(v, clamped(near[1]))) {
            probs |= (uint32_t)mc[cnt[2] * 4 + 2] << 16;
            mode = 2;
            if (!pack_same(v, clamped(near[2]))) {
                probs |= (uint32_t)mc[3] << 24;             // the SPLITMV count is always 0
                mode = 3;
                const PackMv best = clamped(cnt[1] >= cnt[0] ? near[1] : near[0]);
                dr = (v.r - best.r) >> 1; dc = (v.c - best.c) >> 1;
                if (dr < -1023 || dr > 1023 || dc < -1023 || dc > 1023) status |= PACK_BAD_VECTOR;
                // what the decoder's clamp_mv_to_umv_border would move
                if (v.c < left - (19 << 3) || v.c > right + (18 << 3) || v.r < top - (19 << 3) || v.r > bottom + (18 << 3)) status |= PACK_CLAMPS;
            }
        }
    }
    uint32_t rec[8] = {nz | (uint32_t)mode << 25, 0, 0, 0, 0, 0, probs, ((uint32_t)dr & 0xffffu) | (uint32_t)dc << 16};
#pragma unroll
    for (int b = 0; b < 25; b++) rec[1 + b / 6] |= (uint32_t)s_end[g][b] << (5 * (b % 6));
    uint4 *out = (uint4 *)(pack_job(scratch, L, job) + (size_t)mb * PACK_RECORD_BYTES);
    out[0] = make_uint4(rec[0], rec[1], rec[2], rec[3]);
    out[1] = make_uint4(rec[4], rec[5], rec[6], rec[7]);
    uint32_t *ctr = pack_counters(scratch, job);
    if (status) atomicOr(&ctr[PACK_CTR_STATUS], status);
    if (!nz) atomicAdd(&ctr[PACK_CTR_SKIPPED], 1u);
    atomicAdd(&ctr[PACK_CTR_MODES + mode], 1u);
}

// ---- the first partition ------------------------------------------------------------------------------------------------------
// RFC 6386 section 17: a vector component in quarter pel, |v| <= 1023, p its 19 probabilities
static __device__ void pack_mv_component(PackCoder &e, int v, const uint8_t *p)
{
    const int x = v < 0 ? -v : v;
    if (x < 8) {
        pack_put(e, 0, p[0]);
        pack_put(e, x >> 2, p[2]);
        pack_put(e, (x >> 1) & 1, p[x < 4 ? 3 : 6]);
        pack_put(e, x & 1, p[x < 4 ? (x < 2 ? 4 : 5) : (x < 6 ? 7 : 8)]);
    } else {
        pack_put(e, 1, p[0]);
        for (int i = 0; i < 3; i++) pack_put(e, (x >> i) & 1, p[9 + i]);
        for (int i = 9; i > 3; i--) pack_put(e, (x >> i) & 1, p[9 + i]);
        if (x & 0xfff0) pack_put(e, (x >> 3) & 1, p[9 + 3]);
    }
    if (x) pack_put(e, v < 0, p[1]);
}

extern "C" __global__ __launch_bounds__(PACK_CODER_THREADS) void vp8_pack_first_kernel(uint8_t *scratch, int jobs, PackLaunch L)
{
    __shared__ uint8_t s_mvc[40];
    if (threadIdx.x < 38) s_mvc[threadIdx.x] = pack_tables::vp8t_default_mv_context[threadIdx.x];
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
    const uint4 *recs = (const uint4 *)area;
#pragma unroll 1
    for (int mb = 0; mb < nmb; mb++) {
        const uint32_t w0 = recs[2 * mb].x;
        const uint4 hi = recs[2 * mb + 1];
        const int mode = (int)(w0 >> 25) & 3;
        pack_put(e, !(w0 & PACK_NZ_MASK), (uint32_t)L.prob_skip);
        pack_put(e, 1, (uint32_t)L.prob_intra);
        pack_put(e, L.ref_frame != 1, (uint32_t)L.prob_last);
        if (L.ref_frame != 1) pack_put(e, L.ref_frame - 2, (uint32_t)L.prob_gf);
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
#define PACK_P(j) ((p[(j) >> 2] >> (8 * ((j) & 3))) & 0xffu)

extern "C" __global__ __launch_bounds__(PACK_CODER_THREADS) void vp8_pack_tokens_kernel(const uint8_t *coef, size_t coef_stride, uint8_t *scratch, int jobs,
                                                                                       PackLaunch L)
{
    __shared__ uint32_t s_coef[96 * PACK_ROW_BYTES / 4];
    __shared__ uint8_t s_cat[32];
    __shared__ uint4 s_block[PACK_CODER_THREADS][2];
    // DCT_CAT1..6: the extra bits' probabilities back to back (RFC 6386 13.2); a category's start and length
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
                    const uint32_t *p = s_coef + ((type * 8 + band) * 3 + ctx) * (PACK_ROW_BYTES / 4);
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

// ---- the frame ----------------------------------------------------------------------------------------------------------------
extern "C" __global__ __launch_bounds__(256) void vp8_pack_assemble_kernel(const uint8_t *scratch, uint8_t *dst, size_t dst_stride, uint32_t *info, PackLaunch L)
{
    const int job = blockIdx.x, nparts = 1 << L.log2_parts;
    const uint32_t *ctr = (const uint32_t *)scratch + (size_t)job * PACK_CTR_DWORDS;
    const uint8_t *area = scratch + L.jobs_off + L.job_bytes * (size_t)job;
    const uint8_t *first_region = area + (size_t)L.mb_cols * L.mb_rows * PACK_RECORD_BYTES;
    uint8_t *out = dst + dst_stride * (size_t)job;
    const uint32_t first = ctr[PACK_CTR_FIRST];
    uint32_t status = ctr[PACK_CTR_STATUS];
    unsigned long long total = 3ull + first + 3ull * (nparts - 1);
    for (int k = 0; k < nparts; k++) total += ctr[PACK_CTR_PARTS + k];
    if (total > L.cap) status |= PACK_OVERFLOW;
    const bool failed = status & (PACK_OVERFLOW | PACK_BAD_VECTOR | PACK_BAD_LEVEL);
    if (threadIdx.x == 0) {
        uint32_t *o = info + (size_t)job * 16;
        o[0] = status;
        o[1] = failed ? 0 : (uint32_t)total;
        o[2] = first;
        for (int k = 0; k < 8; k++) o[3 + k] = k < nparts ? ctr[PACK_CTR_PARTS + k] : 0;
        o[11] = ctr[PACK_CTR_SKIPPED];
        for (int k = 0; k < 4; k++) o[12 + k] = ctr[PACK_CTR_MODES + k];
    }
    if (failed) return;
    if (threadIdx.x == 0) {
        const uint32_t tag = 1u | (uint32_t)L.version << 1 | (uint32_t)L.show_frame << 4 | first << 5;
        out[0] = (uint8_t)tag; out[1] = (uint8_t)(tag >> 8); out[2] = (uint8_t)(tag >> 16);
        for (int k = 0; k < nparts - 1; k++) {
            const uint32_t s = ctr[PACK_CTR_PARTS + k];
            uint8_t *t = out + 3 + first + 3 * k;
            t[0] = (uint8_t)s; t[1] = (uint8_t)(s >> 8); t[2] = (uint8_t)(s >> 16);
        }
    }
    for (uint32_t i = threadIdx.x; i < first; i += 256) out[3 + i] = first_region[i];
    size_t at = 3 + (size_t)first + 3 * (size_t)(nparts - 1);
    for (int k = 0; k < nparts; k++) {
        const uint32_t s = ctr[PACK_CTR_PARTS + k];
        const uint8_t *region = first_region + L.first_cap + (size_t)L.part_cap * k;
        for (uint32_t i = threadIdx.x; i < s; i += 256) out[at + i] = region[i];
        at += s;
    }
}
