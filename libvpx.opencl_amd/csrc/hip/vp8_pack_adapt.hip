// The kernels vp8hip_frames_pack_adapt_async adds to vp8_pack.hip's (include/vp8hip.h has the definition, vp8hip_pack.hip the plan):
// each frame coded with probabilities fitted to its own counts by the reference encoder's rules.  Between the plan kernel and the
// assemble kernel, both vp8_pack.hip's as they stand:
//   vp8_pack_count_kernel         parallel: a lane a block walks the block's tokens from the record's end and the levels and counts
//                                 them by (type, band, context, token); a lane a NEWMV macroblock counts the branches of its two
//                                 coded components.  Four per-wave sub-histograms of 1216 counters in LDS, LDS integer atomics
//                                 without return, then one global integer atomic per non-zero counter into the job's counts:
//                                 vp8_hist.hip's shape.  blockIdx.y is the job: a workgroup never holds two jobs' counts.
//   vp8_pack_choose_kernel        a workgroup a job, a lane a probability: branch counts, the fitted probability, the saving, the
//                                 update flag and the effective byte; lane 0 the header probabilities and the sums of info[16..19].
//   vp8_pack_first_adapt_kernel   \ vp8_pack_tokens.hip.h's pack_first<true> and pack_tokens<PACK_TOKENS_OWN>: the probability section
//   vp8_pack_tokens_adapt_kernel  / of the header on the device, the job's own vector and coefficient tables.
//   vp8_pack_adapt_info_kernel    the call's 32 uint32 a job from the assemble kernel's 16 and the choose kernel's 4.
// Integer adds commute: the same bits in every run.  Levels and vector differences are data here, never addresses: a level of any
// size counts as DCT_CAT6 and a difference by its low ten magnitude bits (the plan kernel's status says where either is refused).
#include <hip/hip_runtime.h>
#define PACK_CODER_INLINE __forceinline__
#include "vp8_pack_tokens.hip.h"

namespace pack_tables {
#include "../host/vp8_enc_tables.c"
}

typedef __attribute__((address_space(3))) unsigned *pack_lds_u32p;
static __device__ __forceinline__ void count_add(uint32_t *h, int bin)
{
    (void)__hip_atomic_fetch_add((pack_lds_u32p)h + bin, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// the branches of a coded vector component (write_component_probs): h[0..1] is_short_ct, [2..3] sign_ct, [4..11] short_ct,
// [12..31] bit_ct[10][2] -- bit 3 counted for every long vector, as the reference does
static __device__ __forceinline__ void count_component(uint32_t *h, int v)
{
    const int x = (v < 0 ? -v : v) & 1023;
    if (x) count_add(h, 2 + (v < 0));
    if (x < 8) {
        count_add(h, 0);
        count_add(h, 4 + x);
    } else {
        count_add(h, 1);
#pragma unroll 1
        for (int k = 0; k < 10; k++) count_add(h, 12 + 2 * k + ((x >> k) & 1));
    }
}

extern "C" __global__ __launch_bounds__(256) void vp8_pack_count_kernel(const uint8_t *coef, size_t coef_stride, uint8_t *scratch, PackLaunch L, PackAdapt A)
{
    __shared__ uint32_t s_hist[4][PACK_ADAPT_COUNT_DWORDS];
#pragma unroll 1
    for (int t = threadIdx.x; t < 4 * PACK_ADAPT_COUNT_DWORDS; t += 256) (&s_hist[0][0])[t] = 0u;
    __syncthreads();
    const int job = blockIdx.y, g = threadIdx.x >> 5, l = threadIdx.x & 31;
    const int cols = L.mb_cols, nmb = L.mb_cols * L.mb_rows;
    const int mb = (int)blockIdx.x * 8 + g;
    uint32_t *h = s_hist[threadIdx.x >> 6];
    if (mb < nmb && l < 26) {
        const uint4 *recs = (const uint4 *)pack_job(scratch, L, job);
        const uint4 lo = recs[2 * mb], hi = recs[2 * mb + 1];
        const uint32_t own = lo.x & PACK_NZ_MASK;
        if (l == 25) {                  // the macroblock's vector, whether it is skipped or not
            if (((lo.x >> 25) & 3) == 3) {
                count_component(h + 1152, (int16_t)(hi.w & 0xffff));
                count_component(h + 1152 + 32, (int16_t)(hi.w >> 16));
            }
        } else if (own) {               // a skipped macroblock codes no token
            const int r = mb / cols, c = mb - r * cols;
            const uint32_t up = r ? recs[2 * (mb - cols)].x & PACK_NZ_MASK : 0, left = c ? recs[2 * (mb - 1)].x & PACK_NZ_MASK : 0;
            const int blk = l, type = blk == 24 ? 1 : blk < 16 ? 0 : 2, first = blk < 16;
            // the context and the end as the token coder takes them
            int ctx = pack_block_ctx(blk, own, up, left);
            const int end = pack_record_end(lo, hi.x, hi.y, blk);
            const uint4 *p = (const uint4 *)(coef + coef_stride * (size_t)job + ((size_t)mb * 25 + blk) * 32);
            const uint4 p0 = p[0], p1 = p[1];
            const uint32_t w[8] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w};
            uint32_t *row = h + type * (8 * 3 * 12);
#pragma unroll
            for (int i = 0; i < 16; i++) {
                if (i >= first && i < end) {
                    const int z = pack_zigzag(i), v = (int16_t)(w[z >> 1] >> (16 * (z & 1)));
                    const int x = v < 0 ? -v : v;
                    const int tok = x < 5 ? x : 5 + pack_category(x);
                    count_add(row, (pack_band(i) * 3 + ctx) * 12 + tok);
                    ctx = x == 0 ? 0 : x == 1 ? 1 : 2;
                }
            }
            const int at = end > first ? end : first;       // the end of block, unless the block ends at step 15
            if (at < 16) count_add(row, (pack_band(at) * 3 + ctx) * 12 + 11);
        }
    }
    __syncthreads();
    uint32_t *out = (uint32_t *)(pack_adapt_job(scratch, A, job) + PACK_ADAPT_COUNTS);
#pragma unroll 1
    for (int t = threadIdx.x; t < PACK_ADAPT_COUNT_DWORDS; t += 256) {
        const uint32_t s = s_hist[0][t] + s_hist[1][t] + s_hist[2][t] + s_hist[3][t];
        if (s) (void)__hip_atomic_fetch_add(out + t, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// vp8_cost_branch: unsigned 32-bit arithmetic, as the reference's
static __device__ __forceinline__ uint32_t cost_branch(uint32_t c0, uint32_t c1, uint32_t p)
{
    return (c0 * pack_tables::vp8t_prob_cost[p] + c1 * pack_tables::vp8t_prob_cost[255 - p]) >> 8;
}

static __device__ __forceinline__ uint32_t sum_of(const uint32_t *c, int from, int to)
{
    uint32_t s = 0;
    for (int i = from; i <= to; i++) s += c[i];
    return s;
}

extern "C" __global__ __launch_bounds__(256) void vp8_pack_choose_kernel(uint8_t *scratch, PackLaunch L, PackAdapt A)
{
    __shared__ uint32_t s_sum[3];       // coefficient probabilities updated, vector probabilities updated, the sum of the positive s
    const int job = blockIdx.x;
    uint8_t *ad = pack_adapt_job(scratch, A, job);
    const uint32_t *cnt = (const uint32_t *)(ad + PACK_ADAPT_COUNTS);
    const uint32_t *ctr = pack_counters(scratch, job);
    const uint8_t *base = A.probs_in ? A.probs_in + A.probs_in_stride * (size_t)job : nullptr;
    // a job the plan refuses: nothing is counted, so nothing is updated
    const bool bad = ctr[PACK_CTR_STATUS] & (PACK_BAD_VECTOR | PACK_BAD_LEVEL);
    if (threadIdx.x < 3) s_sum[threadIdx.x] = 0;
    __syncthreads();
#pragma unroll 1
    for (int i = threadIdx.x; i < PACK_PROBS_BYTES; i += 256) {
        uint32_t eff = 0;
        int u = 0;
        if (i < 1056) {
            // vp8_tree_probs_from_distribution(12, vp8_coef_encodings, vp8_coef_tree, ..., 256, 1) for node i % 11 of the context:
            // tokens 0 ZERO, 1..4, 5..10 DCT_CAT1..6, 11 the end of block
            const int ctxrow = i / 11, node = i - ctxrow * 11;
            const uint32_t *c = cnt + ctxrow * 12;
            uint32_t c0, c1;
            switch (node) {
            case 0: c0 = c[11]; c1 = sum_of(c, 0, 10); break;
            case 1: c0 = c[0]; c1 = sum_of(c, 1, 10); break;
            case 2: c0 = c[1]; c1 = sum_of(c, 2, 10); break;
            case 3: c0 = sum_of(c, 2, 4); c1 = sum_of(c, 5, 10); break;
            case 4: c0 = c[2]; c1 = c[3] + c[4]; break;
            case 5: c0 = c[3]; c1 = c[4]; break;
            case 6: c0 = c[5] + c[6]; c1 = sum_of(c, 7, 10); break;
            case 7: c0 = c[5]; c1 = c[6]; break;
            case 8: c0 = c[7] + c[8]; c1 = c[9] + c[10]; break;
            case 9: c0 = c[7]; c1 = c[8]; break;
            default: c0 = c[9]; c1 = c[10]; break;
            }
            if (bad) c0 = c1 = 0;
            const uint32_t tot = c0 + c1;
            uint32_t newp = 128;
            if (tot) {
                const uint32_t p = (c0 * 256u + (tot >> 1)) / tot;
                newp = p < 256 ? (p ? p : 1) : 255;
            }
            const uint32_t oldp = base ? base[i] : pack_tables::vp8t_default_coef_probs[i];
            const uint32_t upd = pack_tables::vp8t_coef_update_probs[i];
            const int update_b = 8 + (((int)pack_tables::vp8t_prob_cost[255 - upd] - (int)pack_tables::vp8t_prob_cost[upd]) >> 8);
            const int s = (int)cost_branch(c0, c1, oldp) - (int)cost_branch(c0, c1, newp) - update_b;
            u = (A.flags & PACK_ADAPT_COEF) && s > 0;
            eff = u ? newp : oldp;
            if (u) {
                atomicAdd(&s_sum[0], 1u);
                atomicAdd(&s_sum[2], (uint32_t)s);
            }
            ad[PACK_ADAPT_ROWS + ctxrow * 12 + node] = (uint8_t)eff;       // the row of the token coder's table: 12 bytes, the last 0
            if (node == 10) ad[PACK_ADAPT_ROWS + ctxrow * 12 + 11] = 0;
        } else if (i < 1056 + 38) {
            // write_component_probs: the branch counts of probability k of a component; calc_prob from the DEFAULT context
            const int j = i - 1056, comp = j >= 19, k = j - 19 * comp;
            const uint32_t *m = cnt + 1152 + 32 * comp, *sh = m + 4;
            uint32_t c0, c1;
            switch (k) {
            case 0: c0 = m[0]; c1 = m[1]; break;
            case 1: c0 = m[2]; c1 = m[3]; break;
            case 2: c0 = sum_of(sh, 0, 3); c1 = sum_of(sh, 4, 7); break;       // vp8_small_mvtree
            case 3: c0 = sh[0] + sh[1]; c1 = sh[2] + sh[3]; break;
            case 4: c0 = sh[0]; c1 = sh[1]; break;
            case 5: c0 = sh[2]; c1 = sh[3]; break;
            case 6: c0 = sh[4] + sh[5]; c1 = sh[6] + sh[7]; break;
            case 7: c0 = sh[4]; c1 = sh[5]; break;
            case 8: c0 = sh[6]; c1 = sh[7]; break;
            default: c0 = m[12 + 2 * (k - 9)]; c1 = m[13 + 2 * (k - 9)]; break;
            }
            if (bad) c0 = c1 = 0;
            const uint32_t tot = c0 + c1;
            uint32_t newp = pack_tables::vp8t_default_mv_context[j];
            if (tot) {
                const uint32_t x = ((c0 * 255u) / tot) & 0xfeu;
                newp = x ? x : 1;
            }
            const uint32_t oldp = base ? base[i] : pack_tables::vp8t_default_mv_context[j];
            const uint32_t upd = pack_tables::vp8t_mv_update_probs[j];
            const int cost = 7 - 1 + (((int)pack_tables::vp8t_prob_cost[255 - upd] - (int)pack_tables::vp8t_prob_cost[upd] + 128) >> 8);
            u = (A.flags & PACK_ADAPT_MV) && (int)cost_branch(c0, c1, oldp) - (int)cost_branch(c0, c1, newp) > cost;
            eff = u ? newp : oldp;
            if (u) atomicAdd(&s_sum[1], 1u);
        }
        ad[PACK_ADAPT_EFF + i] = (uint8_t)eff;
        ad[PACK_ADAPT_FLAG + i] = (uint8_t)u;
        if (A.probs_out) A.probs_out[(size_t)job * PACK_PROBS_BYTES + i] = (uint8_t)eff;
    }
    if (A.counts) {
#pragma unroll 1
        for (int t = threadIdx.x; t < PACK_ADAPT_COUNT_DWORDS; t += 256) A.counts[(size_t)job * PACK_ADAPT_COUNT_DWORDS + t] = bad ? 0u : cnt[t];
    }
    __syncthreads();
    if (threadIdx.x) return;
    const uint32_t nmb = (uint32_t)(L.mb_cols * L.mb_rows);
    uint32_t skip = (uint32_t)L.prob_skip;
    if ((A.flags & PACK_ADAPT_SKIP) && !bad) {
        skip = (nmb - ctr[PACK_CTR_SKIPPED]) * 256u / nmb;
        skip = skip < 1 ? 1 : skip > 255 ? 255 : skip;
    }
    uint32_t *hdr = (uint32_t *)(ad + PACK_ADAPT_HDR);
    hdr[0] = s_sum[0]; hdr[1] = s_sum[1]; hdr[PACK_ADAPT_HDR_SKIP] = skip; hdr[3] = s_sum[2];
    hdr[PACK_ADAPT_HDR_INTRA] = (uint32_t)L.prob_intra; hdr[PACK_ADAPT_HDR_LAST] = (uint32_t)L.prob_last; hdr[PACK_ADAPT_HDR_GF] = (uint32_t)L.prob_gf;
    hdr[7] = 0;
}

// ---- the two coders with every job's own tables ------------------------------------------------------------------------------------
extern "C" __global__ __launch_bounds__(PACK_CODER_THREADS) void vp8_pack_first_adapt_kernel(uint8_t *scratch, int jobs, PackLaunch L, PackAdapt A)
{
    pack_first<true>(scratch, jobs, L, A);
}

extern "C" __global__ __launch_bounds__(PACK_CODER_THREADS) void vp8_pack_tokens_adapt_kernel(const uint8_t *coef, size_t coef_stride, uint8_t *scratch,
                                                                                             int jobs, PackLaunch L, PackAdapt A)
{
    pack_tokens<PACK_TOKENS_OWN>(coef, coef_stride, scratch, jobs, L, A);
}

// a lane an entry: [0..15] the assemble kernel's, [16..19] the choose kernel's (0 for a job the plan refuses), the rest 0
extern "C" __global__ __launch_bounds__(256) void vp8_pack_adapt_info_kernel(const uint8_t *scratch, int jobs, PackAdapt A)
{
    const int t = (int)(blockIdx.x * 256 + threadIdx.x), job = t >> 5, k = t & 31;
    if (job >= jobs) return;
    const uint32_t *made = (const uint32_t *)(scratch + A.info_off) + (size_t)job * 16;
    const uint32_t *hdr = (const uint32_t *)(scratch + A.adapt_off + (size_t)PACK_ADAPT_JOB_BYTES * job + PACK_ADAPT_HDR);
    uint32_t v = 0;
    if (k < 16) v = made[k];
    else if (k < 20 && !(made[0] & (PACK_BAD_VECTOR | PACK_BAD_LEVEL))) v = hdr[k - 16];
    A.info[(size_t)job * 32 + k] = v;
}
