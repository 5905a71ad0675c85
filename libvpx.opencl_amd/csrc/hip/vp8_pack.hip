// The kernels of vp8hip_frames_pack_async (include/vp8hip.h has the definition, vp8hip_pack.hip the plan): compressed VP8 inter
// frames from frames_quant's levels and vectors.
//   vp8_pack_plan_kernel      parallel: a lane a block finds the block's end and checks its levels; a lane a macroblock finds the
//                             skip flag, the mode among ZEROMV / NEARESTMV / NEARMV / NEWMV, the coded difference and the vector
//                             checks, and leaves the macroblock's record (vp8_pack.hip.h) in the scratch.
//   vp8_pack_first_kernel     a lane a job: the first partition behind the header the host coded (vp8hip_pack_header).
//   vp8_pack_tokens_kernel    a lane a token partition: the tokens of macroblock rows part, part + parts, ...
//   vp8_pack_assemble_kernel  a workgroup a job: tag, partitions and size table into the caller's memory, the job's info.
// The two coder kernels are launches of their own because their lanes do very different amounts of work and the lanes of a wave go
// through their loops together.  The bool coder is in vp8_pack_coder.hip.h; the bodies of the coder kernels, the plan's scan and
// record store and the assemble body are in vp8_pack_tokens.hip.h, shared with vp8_pack_adapt.hip and vp8_pack_key.hip: here the
// kernels are made for the default tables.
#include <hip/hip_runtime.h>
#include "vp8_pack_tokens.hip.h"

// ---- the plan -----------------------------------------------------------------------------------------------------------------
struct PackMv { int r, c; };
static __device__ __forceinline__ bool pack_same(PackMv a, PackMv b) { return a.r == b.r && a.c == b.c; }
static __device__ __forceinline__ int pack_clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

extern "C" __global__ __launch_bounds__(256) void vp8_pack_plan_kernel(const uint8_t *mv, size_t mv_stride, const uint8_t *coef, size_t coef_stride,
                                                                       uint8_t *scratch, PackLaunch L)
{
    __shared__ uint8_t s_end[8][32];
    const int job = blockIdx.y, g = threadIdx.x >> 5, l = threadIdx.x & 31;
    const int cols = L.mb_cols, nmb = L.mb_cols * L.mb_rows;
    const int mb = (int)blockIdx.x * 8 + g;
    uint32_t nz;
    bool any_bad;
    // position 0 of a luma block is not coded: the Y2 block carries it
    pack_plan_scan(coef + coef_stride * (size_t)job, mb, l < 16 ? 1 : 0, mb < nmb && l < 25, s_end[g], nz, any_bad);
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
    pack_record_store(scratch, L, job, mb, rec, s_end[g], status);
    atomicAdd(&pack_counters(scratch, job)[PACK_CTR_MODES + mode], 1u);
}

// ---- the two coders with the default tables -----------------------------------------------------------------------------------
extern "C" __global__ __launch_bounds__(PACK_CODER_THREADS) void vp8_pack_first_kernel(uint8_t *scratch, int jobs, PackLaunch L)
{
    pack_first<false>(scratch, jobs, L);
}

extern "C" __global__ __launch_bounds__(PACK_CODER_THREADS) void vp8_pack_tokens_kernel(const uint8_t *coef, size_t coef_stride, uint8_t *scratch, int jobs,
                                                                                       PackLaunch L)
{
    pack_tokens<PACK_TOKENS_DEFAULT>(coef, coef_stride, scratch, jobs, L);
}

// ---- the frame ----------------------------------------------------------------------------------------------------------------
// three bytes in front: the tag with bit 0 set
extern "C" __global__ __launch_bounds__(256) void vp8_pack_assemble_kernel(const uint8_t *scratch, uint8_t *dst, size_t dst_stride, uint32_t *info, PackLaunch L)
{
    pack_assemble<3>(
        scratch, dst, dst_stride, info, L, PACK_OVERFLOW | PACK_BAD_VECTOR | PACK_BAD_LEVEL,
        [](uint32_t *o, const uint32_t *ctr) {
            for (int k = 0; k < 4; k++) o[12 + k] = ctr[PACK_CTR_MODES + k];
        },
        [&](uint8_t *out, uint32_t first) {
            const uint32_t tag = 1u | (uint32_t)L.version << 1 | (uint32_t)L.show_frame << 4 | first << 5;
            out[0] = (uint8_t)tag; out[1] = (uint8_t)(tag >> 8); out[2] = (uint8_t)(tag >> 16);
        });
}
