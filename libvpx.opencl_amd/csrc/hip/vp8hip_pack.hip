// vp8hip_frames_pack_async, vp8hip_pack_bound and vp8hip_pack_header, and vp8hip_frames_pack_adapt_async with its bound, header
// prefix and default set (include/vp8hip.h): compressed VP8 inter frames from frames_quant's levels and vectors, in the caller's
// device memory.  The checks and the plan are made here, once per call, by one function for both calls; the kernels are in
// vp8_pack.hip and vp8_pack_adapt.hip.  The frame header is coded on the host, once per distinct qindex, and travels with its coder state
// in the arguments of the launches (PackLaunch), so a call of many jobs is cut where those are full -- and where the scratch, the
// buffer the RGB call keeps, would pass PACK_SCRATCH_MAX.  vp8hip_frames_pack_key_async with its header, the key frames from
// frames_intra's modes and levels, is at the end.  What the three calls do alike stands once: the shared parameter checks and header
// segment (pack_shared_params_ok, host_head_common, host_head_state), the bound of a PackKind, and the plan's checks, size fields,
// scratch and groups (pack_check_q_cap, pack_check_spans, pack_group_plan, pack_group_heads); the two lists of launches are written out.
#include "vp8hip_ctx.hip.h"
#include "vp8_pack.hip.h"

extern "C" __global__ void vp8_pack_plan_kernel(const uint8_t *mv, size_t mv_stride, const uint8_t *coef, size_t coef_stride, uint8_t *scratch, PackLaunch L);
extern "C" __global__ void vp8_pack_first_kernel(uint8_t *scratch, int jobs, PackLaunch L);
extern "C" __global__ void vp8_pack_tokens_kernel(const uint8_t *coef, size_t coef_stride, uint8_t *scratch, int jobs, PackLaunch L);
extern "C" __global__ void vp8_pack_assemble_kernel(const uint8_t *scratch, uint8_t *dst, size_t dst_stride, uint32_t *info, PackLaunch L);
// vp8_pack_adapt.hip
extern "C" __global__ void vp8_pack_count_kernel(const uint8_t *coef, size_t coef_stride, uint8_t *scratch, PackLaunch L, PackAdapt A);
extern "C" __global__ void vp8_pack_choose_kernel(uint8_t *scratch, PackLaunch L, PackAdapt A);
extern "C" __global__ void vp8_pack_first_adapt_kernel(uint8_t *scratch, int jobs, PackLaunch L, PackAdapt A);
extern "C" __global__ void vp8_pack_tokens_adapt_kernel(const uint8_t *coef, size_t coef_stride, uint8_t *scratch, int jobs, PackLaunch L, PackAdapt A);
extern "C" __global__ void vp8_pack_adapt_info_kernel(const uint8_t *scratch, int jobs, PackAdapt A);
// vp8_pack_key.hip
extern "C" __global__ void vp8_pack_key_plan_kernel(const uint8_t *coef, size_t coef_stride, uint8_t *scratch, PackLaunch L, PackKey K);
extern "C" __global__ void vp8_pack_key_y2_kernel(uint8_t *scratch, int jobs, PackLaunch L);
extern "C" __global__ void vp8_pack_key_first_kernel(uint8_t *scratch, int jobs, PackLaunch L);
extern "C" __global__ void vp8_pack_key_tokens_kernel(const uint8_t *coef, size_t coef_stride, uint8_t *scratch, int jobs, PackLaunch L);
extern "C" __global__ void vp8_pack_key_assemble_kernel(const uint8_t *scratch, uint8_t *dst, size_t dst_stride, uint32_t *info, PackLaunch L, PackKey K);

#define PACK_SCRATCH_MAX ((size_t)2 << 30)      // the scratch of a launch group: at most this much (one job at least)
#define PACK_PART_LIMIT (((size_t)1 << 24) - 16) // the size table has 24 bits for a token partition

static_assert(sizeof(vp8hip_pack_head) == sizeof(PackHead) && offsetof(vp8hip_pack_head, bytes) == offsetof(PackHead, bytes) &&
              VP8HIP_PACK_HEAD_MAX == PACK_HEAD_BYTES, "");
static_assert(sizeof(PackLaunch) + sizeof(PackAdapt) <= 3072, "the launch's arguments");
static_assert(sizeof(vp8hip_pack_probs) == PACK_PROBS_BYTES && offsetof(vp8hip_pack_probs, mvc) == 1056, "");
static_assert(VP8HIP_ADAPT_COEF == PACK_ADAPT_COEF && VP8HIP_ADAPT_MV == PACK_ADAPT_MV && VP8HIP_ADAPT_SKIP == PACK_ADAPT_SKIP &&
              VP8HIP_ADAPT_REF == PACK_ADAPT_REF, "");
static_assert(VP8HIP_PACK_BAD_MODE == PACK_BAD_MODE && sizeof(PackLaunch) + sizeof(PackKey) <= 3072, "");

// RFC 6386 section 7.3 as tests/vp8_writer.py's BoolEncoder states it: a carry walks back through the bytes written
struct HostBool {
    uint8_t *out;
    size_t n, cap;
    uint32_t range = 255, bottom = 0;
    int bit_count = 24;
    bool over = false;
    void carry()
    {
        size_t i = n;
        while (i > 0 && out[i - 1] == 255) out[--i] = 0;
        if (i > 0) out[i - 1]++;
    }
    void put(int bit, int prob)
    {
        const uint32_t split = 1 + (((range - 1) * (uint32_t)prob) >> 8);
        if (bit) { bottom += split; range -= split; } else range = split;
        while (range < 128) {
            range <<= 1;
            if (bottom & (1u << 31)) carry();
            bottom <<= 1;
            if (!--bit_count) {
                if (n < cap) out[n++] = (uint8_t)(bottom >> 24); else over = true;
                bottom &= (1u << 24) - 1;
                bit_count = 8;
            }
        }
    }
    void literal(int value, int bits) { for (int i = bits - 1; i >= 0; i--) put((value >> i) & 1, 128); }
};

static bool in(int v, int lo, int hi) { return v >= lo && v <= hi; }

// what both parameter structs hold and the calls refuse alike (the qindex aside)
template <class P>
static bool pack_shared_params_ok(const P *p)
{
    if (!p) return false;
    for (int k = 0; k < 5; k++)
        if (!in(p->delta[k], -15, 15)) return false;
    return in(p->show_frame, 0, 1) && in(p->filter_type, 0, 1) && in(p->version, 0, 3) && in(p->filter_level, 0, 63) && in(p->sharpness, 0, 7) &&
           in(p->log2_parts, 0, 3) && in(p->prob_skip_false, 1, 255);
}

// what the call refuses on p alone
static bool pack_params_ok(const vp8hip_pack *p)
{
    if (!pack_shared_params_ok(p)) return false;
    for (int f : {p->refresh_last, p->refresh_golden, p->refresh_alt, p->sign_bias_golden, p->sign_bias_alt})
        if (!in(f, 0, 1)) return false;
    for (int pr : {p->prob_intra, p->prob_last, p->prob_gf})
        if (!in(pr, 1, 255)) return false;
    return in(p->ref_frame, 1, 3) && in(p->copy_buffer_to_gf, 0, 2) && in(p->copy_buffer_to_arf, 0, 2);
}

static bool pack_key_params_ok(const vp8hip_pack_key *p) { return pack_shared_params_ok(p) && in(p->color_space, 0, 1) && in(p->clamping_type, 0, 1); }

// a frame header from segmentation_enabled through the five quantiser deltas: an inter frame's and a key frame's alike
template <class P>
static void host_head_common(HostBool &e, const P *p, int qindex)
{
    e.literal(0, 1);                                         // segmentation_enabled
    e.literal(p->filter_type, 1);
    e.literal(p->filter_level, 6);
    e.literal(p->sharpness, 3);
    e.literal(0, 1);                                         // mode_ref_lf_delta_enabled
    e.literal(p->log2_parts, 2);
    e.literal(qindex, 7);
    for (int k = 0; k < 5; k++) {
        const int d = p->delta[k];
        e.put(d != 0, 128);
        if (d) { e.literal(d < 0 ? -d : d, 4); e.put(d < 0, 128); }
    }
}

static void host_head_no_coef_update(HostBool &e)
{
    for (int i = 0; i < 1056; i++) e.put(0, pack_tables::vp8t_coef_update_probs[i]);
    e.literal(1, 1);                                         // mb_no_coeff_skip
}

// the coder's state where the header ends, as the device's coder continues from it: -1 where the header did not fit
static int host_head_state(const HostBool &e, vp8hip_pack_head *out)
{
    if (e.over) return -1;
    out->bottom = e.bottom; out->range = e.range; out->bit_count = (uint32_t)e.bit_count; out->nbytes = (uint32_t)e.n;
    size_t i = e.n;
    while (i > 0 && out->bytes[i - 1] == 255) i--;
    out->cache = i ? out->bytes[i - 1] : -1;
    out->settled = i ? (uint32_t)(i - 1) : 0;
    out->pending = (uint32_t)(e.n - i);
    return 0;
}

// the header through refresh_last (prefix: vp8hip_pack_header_prefix) or to where the per-macroblock data begin, with no update
// (vp8hip_pack_header), and the coder's state there
static int pack_header_to(const vp8hip_pack *p, int qindex, int refresh_entropy_probs, bool prefix, vp8hip_pack_head *out)
{
    if (!out || !pack_params_ok(p) || !in(qindex, 0, 127) || !in(refresh_entropy_probs, 0, 1)) return -2;
    memset(out, 0, sizeof *out);
    HostBool e;
    e.out = out->bytes; e.n = 0; e.cap = sizeof out->bytes;
    host_head_common(e, p, qindex);
    e.literal(p->refresh_golden, 1);
    e.literal(p->refresh_alt, 1);
    if (!p->refresh_golden) e.literal(p->copy_buffer_to_gf, 2);
    if (!p->refresh_alt) e.literal(p->copy_buffer_to_arf, 2);
    e.literal(p->sign_bias_golden, 1);
    e.literal(p->sign_bias_alt, 1);
    e.literal(refresh_entropy_probs, 1);
    e.literal(p->refresh_last, 1);
    if (!prefix) {
        host_head_no_coef_update(e);
        e.literal(p->prob_skip_false, 8);
        e.literal(p->prob_intra, 8);
        e.literal(p->prob_last, 8);
        e.literal(p->prob_gf, 8);
        e.literal(0, 2);                                     // the intra 16x16 and chroma probabilities stay
        for (int i = 0; i < 38; i++) e.put(0, pack_tables::vp8t_mv_update_probs[i]);
    }
    return host_head_state(e, out);
}

extern "C" int vp8hip_pack_header(const vp8hip_pack *p, int qindex, vp8hip_pack_head *out) { return pack_header_to(p, qindex, 1, false, out); }

extern "C" int vp8hip_pack_header_prefix(const vp8hip_pack *p, int qindex, int refresh_entropy_probs, vp8hip_pack_head *out)
{
    return pack_header_to(p, qindex, refresh_entropy_probs, true, out);
}

extern "C" void vp8hip_pack_probs_default(vp8hip_pack_probs *out)
{
    if (!out) return;
    memset(out, 0, sizeof *out);
    memcpy(out->coef, pack_tables::vp8t_default_coef_probs, sizeof out->coef);
    memcpy(out->mvc, pack_tables::vp8t_default_mv_context, sizeof out->mvc);
}

// What the three kinds of frame differ by in size: the bytes in front of the first partition, the worst case of a macroblock in
// the first partition, and the bytes of the probability section where the device codes it.
struct PackKind { size_t header, mb_first, update; };
static const PackKind PACK_INTER = {3, PACK_MB_FIRST_BYTES, 0}, PACK_INTER_ADAPT = {3, PACK_MB_FIRST_BYTES, PACK_ADAPT_UPDATE_BYTES},
                      PACK_KEYFRAME = {PACK_KEY_HEADER_BYTES, PACK_KEY_MB_FIRST_BYTES, 0};

static size_t pack_first_bound(size_t nmb, const PackKind &kind) { return PACK_HEAD_BYTES + 4 + kind.update + kind.mb_first * nmb + PACK_FLUSH_BYTES; }

static size_t pack_bound(const vp8hip_ctx *c, int log2_parts, const PackKind &kind)
{
    if (!c || !c->width || log2_parts < 0 || log2_parts > 3) return 0;
    const size_t nmb = (size_t)c->dg.mb_cols * c->dg.mb_rows, parts = (size_t)1 << log2_parts;
    return align_up(kind.header + pack_first_bound(nmb, kind) + 3 * (parts - 1) + PACK_MB_TOKEN_BYTES * nmb + PACK_FLUSH_BYTES * parts, 16);
}

extern "C" size_t vp8hip_pack_bound(const vp8hip_ctx *c, int log2_parts) { return pack_bound(c, log2_parts, PACK_INTER); }
extern "C" size_t vp8hip_pack_adapt_bound(const vp8hip_ctx *c, int log2_parts) { return pack_bound(c, log2_parts, PACK_INTER_ADAPT); }
extern "C" size_t vp8hip_pack_key_bound(const vp8hip_ctx *c, int log2_parts) { return pack_bound(c, log2_parts, PACK_KEYFRAME); }

// ---- what the calls' plans share ------------------------------------------------------------------------------------------------------
// the quantiser and cap: every call's checks behind its parameters, in this order
static int pack_check_q_cap(vp8hip_ctx *c, const char *who, int n, int qindex, const uint8_t *job_qindex, size_t cap, size_t dst_stride)
{
    if (!job_qindex && (qindex < 0 || qindex > 127)) return fail(c, -2, "%s: qindex %d (0..127)", who, qindex);
    if (job_qindex)
        for (int i = 0; i < n; i++)
            if (job_qindex[i] > 127) return fail(c, -2, "%s: job_qindex[%d] = %d (0..127)", who, i, job_qindex[i]);
    if (cap < 16 || cap % 16 || cap > dst_stride) return fail(c, -2, "%s: cap %zu (a multiple of 16, 16 .. the stride %zu)", who, cap, dst_stride);
    return 0;
}

// A call's memory, the outputs first: every span that is given checked by name, then the `outputs` against each other and against
// the inputs.
struct PackSpan { const void *p; size_t stride, size, align; int n; const char *name; };
static int pack_check_spans(vp8hip_ctx *c, const char *who, const PackSpan *t, int count, int outputs)
{
    for (int i = 0; i < count; i++)
        if (t[i].p)
            if (int rc = vp8hip_check_named_dst(c, who, t[i].name, t[i].p, t[i].stride, t[i].size, t[i].align, t[i].n)) return rc;
    for (int i = 0; i < outputs; i++)
        for (int j = i + 1; j < count; j++)
            if (t[i].p && t[j].p && vp8hip_spans_overlap(t[i].p, t[i].stride, t[i].n, t[j].p, t[j].stride, t[j].n))
                return fail(c, -2, "%s: %s and %s overlap", who, t[i].name, t[j].name);
    return 0;
}

// The size fields of L (log2_parts is set), the jobs of a launch group and the scratch, grown to hold them.  No frame is longer
// than the bound, no first partition than its own, no token partition than that of the most rows one has.  A: the adapt call's
// areas behind the jobs', or NULL.
static int pack_group_plan(vp8hip_ctx *c, const char *who, int n, const PackKind &kind, size_t cap, PackLaunch &L, PackAdapt *A, size_t *jobs_a_group)
{
    const size_t nmb = (size_t)c->dg.mb_cols * c->dg.mb_rows, parts = (size_t)1 << L.log2_parts;
    const size_t bound = pack_bound(c, L.log2_parts, kind), frame_limit = kind.header + PACK_FIRST_LIMIT + 24 + 8 * PACK_PART_LIMIT;
    const size_t eff = cap < bound ? cap : bound;
    const size_t part_rows = ((size_t)c->dg.mb_rows + parts - 1) / parts;
    const size_t part_bound = PACK_MB_TOKEN_BYTES * part_rows * c->dg.mb_cols + PACK_FLUSH_BYTES;
    auto least = [](size_t a, size_t b, size_t d) { a = a < b ? a : b; return a < d ? a : d; };
    L.cap = (uint32_t)(eff < frame_limit ? eff : frame_limit);
    L.first_cap = (uint32_t)align_up(least(pack_first_bound(nmb, kind), eff, PACK_FIRST_LIMIT), 16);
    L.part_cap = (uint32_t)align_up(least(part_bound, eff, PACK_PART_LIMIT), 16);
    L.job_bytes = PACK_RECORD_BYTES * nmb + L.first_cap + parts * L.part_cap;
    const size_t adapt_job = A ? PACK_ADAPT_JOB_BYTES + 64 : 0;  // (the adapt area and the assemble kernel's info)
    size_t chunk = n < PACK_MAX_JOBS ? n : PACK_MAX_JOBS;
    const size_t fit = (PACK_SCRATCH_MAX - (A ? 512 : 0)) / (L.job_bytes + 4 * PACK_CTR_DWORDS + adapt_job);     // (512: the two roundings to 256)
    if (chunk > fit) chunk = fit < 1 ? 1 : fit;
    L.jobs_off = align_up(chunk * 4 * PACK_CTR_DWORDS, 256);
    size_t need = L.jobs_off + chunk * L.job_bytes;
    if (A) {
        A->adapt_off = align_up(need, 256);
        A->info_off = A->adapt_off + chunk * PACK_ADAPT_JOB_BYTES;
        need = A->info_off + chunk * 64;
    }
    // (launches in flight read the scratch: hipFree waits for them)
    if (c->d_rgb.grow(need) != hipSuccess) return fail(c, -1, "%s: no device memory for %zu bytes of scratch", who, need);
    *jobs_a_group = chunk;
    return 0;
}

// The jobs of the group that begins at job i0: up to `chunk`, cut where a ninth distinct qindex would come.  header(q, &h) codes
// the frame header of qindex q; L.heads and L.head_of are filled.  Returns the number of jobs, or a negative code with the error set.
template <class Header>
static int pack_group_heads(vp8hip_ctx *c, const char *who, int n, int i0, size_t chunk, int qindex, const uint8_t *job_qindex, PackLaunch &L, Header header)
{
    int m = 0, heads = 0, qof[PACK_MAX_HEADS];
    for (; i0 + m < n && m < (int)chunk; m++) {
        const int q = job_qindex ? job_qindex[i0 + m] : qindex;
        int k = 0;
        while (k < heads && qof[k] != q) k++;
        if (k == heads) {
            if (heads == PACK_MAX_HEADS) break;
            qof[heads] = q;
            vp8hip_pack_head h;
            if (header(q, &h)) return fail(c, -1, "%s: the frame header does not fit %d bytes", who, VP8HIP_PACK_HEAD_MAX);
            memcpy(&L.heads[heads++], &h, sizeof h);
        }
        L.head_of[m] = (uint8_t)k;
    }
    return m;
}

// The plan of both calls.  a == NULL: vp8hip_frames_pack_async -- the four kernels of vp8_pack.hip, info 16 uint32 a job.  Else
// vp8hip_frames_pack_adapt_async: count and choose behind the plan kernel, the coders' ADAPT variants, and the assemble kernel's
// 16 uint32 go to the scratch, from where the info kernel makes the call's 32.
static int pack_frames(vp8hip_ctx *c, const char *who, int n, const vp8hip_pack *p, const vp8hip_pack_adapt *a, const void *mv, size_t mv_stride,
                       const void *coef, size_t coef_stride, void *dst, size_t dst_stride, size_t cap, void *info, void *counts, void *probs_out)
{
    if (!c || n < 1 || !p || !coef || !dst || !info || !c->width) return fail(c, -2, "%s: bad arguments", who);
    if (!pack_params_ok(p))
        return fail(c, -2, "%s: version %d (0..3), flags %d %d %d %d %d %d %d (0, 1), filter level %d (0..63), sharpness %d (0..7), deltas %d %d %d %d %d "
                    "(-15..15), ref_frame %d (1..3), buffer copies %d %d (0..2), log2_parts %d (0..3), probabilities %d %d %d %d (1..255)", who,
                    p->version, p->show_frame, p->filter_type, p->refresh_last, p->refresh_golden, p->refresh_alt, p->sign_bias_golden,
                    p->sign_bias_alt, p->filter_level, p->sharpness, p->delta[0], p->delta[1], p->delta[2], p->delta[3], p->delta[4], p->ref_frame,
                    p->copy_buffer_to_gf, p->copy_buffer_to_arf, p->log2_parts, p->prob_skip_false, p->prob_intra, p->prob_last, p->prob_gf);
    if (int rc = pack_check_q_cap(c, who, n, p->qindex, p->job_qindex, cap, dst_stride)) return rc;
    if (a && (!in(a->flags, 0, 15) || !in(a->refresh_entropy_probs, 0, 1)))
        return fail(c, -2, "%s: flags %d (VP8HIP_ADAPT_* bits), refresh_entropy_probs %d (0, 1)", who, a->flags, a->refresh_entropy_probs);
    const size_t nmb = (size_t)c->dg.mb_cols * c->dg.mb_rows, info_bytes = a ? 128 : 64;
    const void *probs_in = a ? a->probs_in : nullptr;
    const bool one_set = a && !a->probs_in_stride;           // stride 0: one baseline for all jobs
    // the outputs first, then the inputs
    const PackSpan t[7] = {
        {dst, dst_stride, cap, 16, n, "dst"}, {info, info_bytes, info_bytes, 4, n, "info"},
        {counts, 4 * PACK_ADAPT_COUNT_DWORDS, 4 * PACK_ADAPT_COUNT_DWORDS, 4, n, "counts"}, {probs_out, PACK_PROBS_BYTES, PACK_PROBS_BYTES, 16, n, "probs_out"},
        {mv, mv_stride, 4 * nmb, 2, n, "mv"}, {coef, coef_stride, 800 * nmb, 16, n, "coef"},
        {probs_in, one_set ? PACK_PROBS_BYTES : a ? a->probs_in_stride : 0, PACK_PROBS_BYTES, 16, one_set ? 1 : n, "probs_in"}};
    if (int rc = pack_check_spans(c, who, t, 7, 4)) return rc;
    HIPCHK(c, hipSetDevice(c->device));

    PackLaunch L;
    memset(&L, 0, sizeof(L));
    const int parts = 1 << p->log2_parts;
    L.mb_cols = c->dg.mb_cols; L.mb_rows = c->dg.mb_rows;
    L.log2_parts = p->log2_parts; L.has_mv = mv != nullptr;
    L.ref_frame = p->ref_frame;
    L.prob_skip = p->prob_skip_false; L.prob_intra = p->prob_intra; L.prob_last = p->prob_last; L.prob_gf = p->prob_gf;
    L.version = p->version; L.show_frame = p->show_frame;
    if (a && (a->flags & VP8HIP_ADAPT_REF)) {
        // vp8_convert_rfct_to_prob of a frame whose macroblocks are all inter on ref_frame: 0 * 255 / n = 0 becomes 1; LAST or GOLDEN
        // n * 255 / n = 255; prob_gf of a frame without GOLDEN and ALTREF macroblocks 128
        L.prob_intra = 1;
        L.prob_last = p->ref_frame == 1 ? 255 : 1;
        L.prob_gf = p->ref_frame == 1 ? 128 : p->ref_frame == 2 ? 255 : 1;
    }
    PackAdapt A;
    memset(&A, 0, sizeof(A));
    size_t chunk;
    if (int rc = pack_group_plan(c, who, n, a ? PACK_INTER_ADAPT : PACK_INTER, cap, L, a ? &A : nullptr, &chunk)) return rc;
    uint8_t *scratch = c->d_rgb;

    for (int i0 = 0; i0 < n;) {
        const int m = pack_group_heads(c, who, n, i0, chunk, p->qindex, p->job_qindex, L, [&](int q, vp8hip_pack_head *h) {
            return pack_header_to(p, q, a ? a->refresh_entropy_probs : 1, a != nullptr, h);
        });
        if (m < 0) return m;
        auto at = [i0](const void *ptr, size_t stride) { return ptr ? (uint8_t *)ptr + stride * (size_t)i0 : nullptr; };
        const dim3 plan_grid((unsigned)((nmb + 7) / 8), (unsigned)m), first_grid((unsigned)((m + 63) / 64)), tokens_grid((unsigned)((m * parts + 63) / 64));
        const uint8_t *mv_at = (const uint8_t *)at(mv, mv_stride), *coef_at = (const uint8_t *)at(coef, coef_stride);
        HIPCHK(c, hipMemsetAsync(scratch, 0, (size_t)m * 4 * PACK_CTR_DWORDS, c->stream));
        hipLaunchKernelGGL(vp8_pack_plan_kernel, plan_grid, dim3(256), 0, c->stream, mv_at, mv_stride, coef_at, coef_stride, scratch, L);
        if (!a) {
            hipLaunchKernelGGL(vp8_pack_first_kernel, first_grid, dim3(64), 0, c->stream, scratch, m, L);
            hipLaunchKernelGGL(vp8_pack_tokens_kernel, tokens_grid, dim3(64), 0, c->stream, coef_at, coef_stride, scratch, m, L);
            hipLaunchKernelGGL(vp8_pack_assemble_kernel, dim3((unsigned)m), dim3(256), 0, c->stream, (const uint8_t *)scratch, at(dst, dst_stride), dst_stride,
                               (uint32_t *)at(info, 64), L);
        } else {
            A.probs_in = (const uint8_t *)at(a->probs_in, a->probs_in_stride);
            A.probs_in_stride = a->probs_in_stride;
            A.info = (uint32_t *)at(info, 128);
            A.counts = (uint32_t *)at(counts, 4 * PACK_ADAPT_COUNT_DWORDS);
            A.probs_out = at(probs_out, PACK_PROBS_BYTES);
            A.flags = a->flags;
            // (the counts of every job's adapt area: the count kernel adds to them)
            HIPCHK(c, hipMemsetAsync(scratch + A.adapt_off, 0, (size_t)m * PACK_ADAPT_JOB_BYTES, c->stream));
            hipLaunchKernelGGL(vp8_pack_count_kernel, plan_grid, dim3(256), 0, c->stream, coef_at, coef_stride, scratch, L, A);
            hipLaunchKernelGGL(vp8_pack_choose_kernel, dim3((unsigned)m), dim3(256), 0, c->stream, scratch, L, A);
            hipLaunchKernelGGL(vp8_pack_first_adapt_kernel, first_grid, dim3(64), 0, c->stream, scratch, m, L, A);
            hipLaunchKernelGGL(vp8_pack_tokens_adapt_kernel, tokens_grid, dim3(64), 0, c->stream, coef_at, coef_stride, scratch, m, L, A);
            hipLaunchKernelGGL(vp8_pack_assemble_kernel, dim3((unsigned)m), dim3(256), 0, c->stream, (const uint8_t *)scratch, at(dst, dst_stride), dst_stride,
                               (uint32_t *)(scratch + A.info_off), L);
            hipLaunchKernelGGL(vp8_pack_adapt_info_kernel, dim3((unsigned)((m * 32 + 255) / 256)), dim3(256), 0, c->stream, (const uint8_t *)scratch, m, A);
        }
        HIPCHK(c, hipGetLastError());
        i0 += m;
    }
    return 0;
}

extern "C" int vp8hip_frames_pack_async(vp8hip_ctx *c, int n, const vp8hip_pack *p, const void *mv, size_t mv_stride, const void *coef,
                                        size_t coef_stride, void *dst, size_t dst_stride, size_t cap, void *info)
{
    return pack_frames(c, "vp8hip_frames_pack_async", n, p, nullptr, mv, mv_stride, coef, coef_stride, dst, dst_stride, cap, info, nullptr, nullptr);
}

extern "C" int vp8hip_frames_pack_adapt_async(vp8hip_ctx *c, int n, const vp8hip_pack *p, const vp8hip_pack_adapt *a, const void *mv, size_t mv_stride,
                                              const void *coef, size_t coef_stride, void *dst, size_t dst_stride, size_t cap, void *info, void *counts,
                                              void *probs_out)
{
    const char *who = "vp8hip_frames_pack_adapt_async";
    if (!a) return fail(c, -2, "%s: bad arguments", who);
    return pack_frames(c, who, n, p, a, mv, mv_stride, coef, coef_stride, dst, dst_stride, cap, info, counts, probs_out);
}

// ---- key frames: vp8hip_frames_pack_key_async, vp8hip_pack_key_header ----------------------------------------------------------------
extern "C" int vp8hip_pack_key_header(const vp8hip_pack_key *p, int qindex, vp8hip_pack_head *out)
{
    if (!out || !pack_key_params_ok(p) || !in(qindex, 0, 127)) return -2;
    memset(out, 0, sizeof *out);
    HostBool e;
    e.out = out->bytes; e.n = 0; e.cap = sizeof out->bytes;
    e.literal(p->color_space, 1);
    e.literal(p->clamping_type, 1);
    host_head_common(e, p, qindex);
    e.literal(1, 1);                                         // refresh_entropy_probs
    host_head_no_coef_update(e);
    e.literal(p->prob_skip_false, 8);
    return host_head_state(e, out);
}

// The checks, the sizes and the groups are pack_frames'; the launches are the kernels of vp8_pack_key.hip.
extern "C" int vp8hip_frames_pack_key_async(vp8hip_ctx *c, int n, const vp8hip_pack_key *p, const void *modes, size_t modes_stride, const void *coef,
                                            size_t coef_stride, void *dst, size_t dst_stride, size_t cap, void *info)
{
    const char *who = "vp8hip_frames_pack_key_async";
    if (!c || n < 1 || !p || !modes || !coef || !dst || !info || !c->width) return fail(c, -2, "%s: bad arguments", who);
    if (!pack_key_params_ok(p))
        return fail(c, -2, "%s: version %d (0..3), flags %d %d %d %d (0, 1), filter level %d (0..63), sharpness %d (0..7), deltas %d %d %d %d %d "
                    "(-15..15), log2_parts %d (0..3), prob_skip_false %d (1..255)", who, p->version, p->show_frame, p->color_space, p->clamping_type,
                    p->filter_type, p->filter_level, p->sharpness, p->delta[0], p->delta[1], p->delta[2], p->delta[3], p->delta[4], p->log2_parts,
                    p->prob_skip_false);
    if (int rc = pack_check_q_cap(c, who, n, p->qindex, p->job_qindex, cap, dst_stride)) return rc;
    const size_t nmb = (size_t)c->dg.mb_cols * c->dg.mb_rows;
    const PackSpan t[4] = {{dst, dst_stride, cap, 16, n, "dst"}, {info, 64, 64, 4, n, "info"}, {modes, modes_stride, 32 * nmb, 4, n, "modes"},
                           {coef, coef_stride, 800 * nmb, 16, n, "coef"}};
    if (int rc = pack_check_spans(c, who, t, 4, 2)) return rc;
    HIPCHK(c, hipSetDevice(c->device));

    PackLaunch L;
    memset(&L, 0, sizeof(L));
    const int parts = 1 << p->log2_parts;
    L.mb_cols = c->dg.mb_cols; L.mb_rows = c->dg.mb_rows;
    L.log2_parts = p->log2_parts;
    L.prob_skip = p->prob_skip_false;
    L.version = p->version; L.show_frame = p->show_frame;
    size_t chunk;
    if (int rc = pack_group_plan(c, who, n, PACK_KEYFRAME, cap, L, nullptr, &chunk)) return rc;
    uint8_t *scratch = c->d_rgb;
    PackKey K;
    K.modes_stride = modes_stride;
    K.width = c->width; K.height = c->height;

    for (int i0 = 0; i0 < n;) {
        const int m = pack_group_heads(c, who, n, i0, chunk, p->qindex, p->job_qindex, L, [&](int q, vp8hip_pack_head *h) { return vp8hip_pack_key_header(p, q, h); });
        if (m < 0) return m;
        const uint8_t *coef_at = (const uint8_t *)coef + coef_stride * (size_t)i0;
        K.modes = (const uint8_t *)modes + modes_stride * (size_t)i0;
        const dim3 plan_grid((unsigned)((nmb + 7) / 8), (unsigned)m);
        HIPCHK(c, hipMemsetAsync(scratch, 0, (size_t)m * 4 * PACK_CTR_DWORDS, c->stream));
        hipLaunchKernelGGL(vp8_pack_key_plan_kernel, plan_grid, dim3(256), 0, c->stream, coef_at, coef_stride, scratch, L, K);
        hipLaunchKernelGGL(vp8_pack_key_y2_kernel, dim3((unsigned)((m * c->dg.mb_cols + 63) / 64)), dim3(64), 0, c->stream, scratch, m, L);
        hipLaunchKernelGGL(vp8_pack_key_first_kernel, dim3((unsigned)((m + 63) / 64)), dim3(64), 0, c->stream, scratch, m, L);
        hipLaunchKernelGGL(vp8_pack_key_tokens_kernel, dim3((unsigned)((m * parts + 63) / 64)), dim3(64), 0, c->stream, coef_at, coef_stride, scratch, m, L);
        hipLaunchKernelGGL(vp8_pack_key_assemble_kernel, dim3((unsigned)m), dim3(256), 0, c->stream, (const uint8_t *)scratch,
                           (uint8_t *)dst + dst_stride * (size_t)i0, dst_stride, (uint32_t *)info + 16 * (size_t)i0, L, K);
        HIPCHK(c, hipGetLastError());
        i0 += m;
    }
    return 0;
}
