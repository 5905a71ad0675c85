// vp8hip_frames_quant_async and vp8hip_quant_factors (include/vp8hip.h): the reference's inter 16x16 encode of every macroblock of a
// picture pair -- predict, subtract, forward DCT and Walsh transform, quantise, and where asked dequantise, inverse-transform and
// add -- as level records, eobs, error planes and a packed I420 reconstruction in the caller's device memory.  The plan and the
// checks are made here, once per call; the kernel is in vp8_quant.hip.  Everything it reads is in the frame buffers as they lie
// (either form, nothing converted), in the caller's vector tensor, or comes with the launch: no device memory is added.  A launch
// carries its jobs and one table per distinct qindex among them in its arguments (QuantLaunch), so a call of many jobs is cut where
// either array is full.
#include "vp8hip_ctx.hip.h"

extern "C" __global__ void vp8_quant_frames_kernel(const uint8_t *raster, size_t fb_stride, const uint8_t *tiles, size_t tile_frame, const uint8_t *mv,
                                                   size_t mv_stride, uint8_t *coef, size_t coef_stride, uint8_t *eobs, size_t eob_stride, uint8_t *stats,
                                                   size_t stats_stride, uint8_t *rec, size_t rec_stride, QuantLaunch L);

#define QUANT_PLANES (VP8HIP_QUANT_ERRY | VP8HIP_QUANT_ERRY2 | VP8HIP_QUANT_ERRUV | VP8HIP_QUANT_EOBS | VP8HIP_QUANT_RECSSE)

extern "C" int vp8hip_quant_factors(int qindex, const int delta[5], vp8hip_quant_table *out)
{
    static const unsigned short dc_q[128] = { VP8_DC_Q_VALUES }, ac_q[128] = { VP8_AC_Q_VALUES };
    static const int zbin_boost[16] = {0, 0, 8, 10, 12, 14, 16, 20, 24, 28, 32, 36, 40, 44, 44, 44};
    static const int none[5] = {0, 0, 0, 0, 0};
    if (!out || qindex < 0 || qindex > 127) return -2;
    if (!delta) delta = none;
    for (int k = 0; k < 5; k++)
        if (delta[k] < -15 || delta[k] > 15) return -2;
    auto qi = [qindex](int d) { const int v = qindex + d; return v < 0 ? 0 : v > 127 ? 127 : v; };
    // vp8_dc_quant, vp8_ac_yquant; vp8_dc2quant, vp8_ac2quant; vp8_dc_uv_quant, vp8_ac_uv_quant (quant_common.c), as vp8hip_dequant_factors
    int y2ac = (ac_q[qi(delta[2])] * 155) / 100; if (y2ac < 8) y2ac = 8;
    int uvdc = dc_q[qi(delta[3])]; if (uvdc > 132) uvdc = 132;
    const int d[3][2] = {{dc_q[qi(delta[0])], ac_q[qindex]}, {dc_q[qi(delta[1])] * 2, y2ac}, {uvdc, ac_q[qi(delta[4])]}};
    const int zf = qindex < 48 ? 84 : 80;                    // qzbin_factors; qrounding_factors is 48 for every qindex
    for (int t = 0; t < 3; t++) {
        for (int k = 0; k < 2; k++) {
            const int v = d[t][k];
            int l = 0;
            for (unsigned u = (unsigned)v; u > 1; u >>= 1) l++;      // invert_quant with improved_quant
            out->quant[t][k] = (int16_t)(1 + (1 << (16 + l)) / v - (1 << 16));
            out->quant_shift[t][k] = (int16_t)l;
            out->quant_fast[t][k] = (int16_t)((1 << 16) / v);
            out->zbin[t][k] = (int16_t)((zf * v + 64) >> 7);
            out->round[t][k] = (int16_t)((48 * v) >> 7);
            out->dequant[t][k] = (int16_t)v;
        }
        for (int i = 0; i < 16; i++) out->zrun_zbin_boost[t][i] = (int16_t)((d[t][i ? 1 : 0] * zbin_boost[i]) >> 7);
    }
    return 0;
}

// the quantiser part of p (vp8hip_intra.hip takes it too): deltas, zero-bin terms, quantizer and stage; job_qindex aside
bool vp8hip_quantiser_ok(const vp8hip_quant *p)
{
    for (int k = 0; k < 5; k++)
        if (p->delta[k] < -15 || p->delta[k] > 15) return false;
    for (int z : {p->zbin_over_quant, p->zbin_mode_boost, p->act_zbin_adj})
        if (z < -QUANT_ZBIN_MAX || z > QUANT_ZBIN_MAX) return false;
    return (p->quantizer == VP8HIP_QUANT_REGULAR || p->quantizer == VP8HIP_QUANT_FAST) &&
           (p->stage == VP8HIP_COEF_LEVELS || p->stage == VP8HIP_COEF_DEQUANT);
}

// what the call refuses on p alone (job_qindex aside)
static bool quant_params_ok(const vp8hip_quant *p)
{
    if (!p || (p->planes & ~(unsigned)QUANT_PLANES)) return false;
    return vp8hip_quantiser_ok(p) && (p->filter == VP8HIP_TFILTER_SIXTAP || p->filter == VP8HIP_TFILTER_BILINEAR);
}

extern "C" size_t vp8hip_quant_coef_size(const vp8hip_ctx *c) { return c && c->width ? (size_t)800 * c->dg.mb_cols * c->dg.mb_rows : 0; }
extern "C" size_t vp8hip_quant_eob_size(const vp8hip_ctx *c) { return c && c->width ? (size_t)32 * c->dg.mb_cols * c->dg.mb_rows : 0; }
extern "C" size_t vp8hip_quant_stats_size(const vp8hip_ctx *c, const vp8hip_quant *p)
{
    if (!c || !c->width || !p || !p->planes || (p->planes & ~(unsigned)QUANT_PLANES)) return 0;
    return (size_t)4 * __builtin_popcount(p->planes) * c->dg.mb_cols * c->dg.mb_rows;
}

// table k of the launch: vp8hip_quant_factors for qindex as it stands, then the three ZBIN_EXTRAs (Y1, Y2, UV) through the `(short)`
void vp8hip_quant_staged_table(short *t, int qindex, const vp8hip_quant *p)
{
    vp8hip_quant_table f;
    vp8hip_quant_factors(qindex, p->delta, &f);
    static_assert(sizeof f == 168 && QUANT_TABLE_SHORTS == 88, "");
    memcpy(t, &f, sizeof f);
    const int all = p->zbin_over_quant + p->zbin_mode_boost + p->act_zbin_adj, y2 = p->zbin_over_quant / 2 + p->zbin_mode_boost + p->act_zbin_adj;
    t[84] = (short)((f.dequant[0][1] * all) >> 7);
    t[85] = (short)((f.dequant[1][1] * y2) >> 7);
    t[86] = (short)((f.dequant[2][1] * all) >> 7);
    t[87] = 0;
}

extern "C" int vp8hip_frames_quant_async(vp8hip_ctx *c, const vp8hip_hist_job *jobs, int n, const vp8hip_quant *p, const void *mv, size_t mv_stride,
                                         void *coef, size_t coef_stride, void *eob, size_t eob_stride, void *stats, size_t stats_stride, void *rec,
                                         size_t rec_stride)
{
    const char *who = "vp8hip_frames_quant_async";
    if (!c || !jobs || n < 1 || !p || (!coef && !eob && !stats && !rec) || !c->width || c->fb.empty()) return fail(c, -2, "%s: bad arguments", who);
    if (int rc = vp8hip_check_pairs(c, who, jobs, n, false)) return rc;
    if (!quant_params_ok(p))
        return fail(c, -2, "%s: deltas %d %d %d %d %d (-15..15), quantizer %d, filter %d, stage %d (0, 1), zero-bin terms %d %d %d (+-%d), planes 0x%x (of 0x%x)",
                    who, p->delta[0], p->delta[1], p->delta[2], p->delta[3], p->delta[4], p->quantizer, p->filter, p->stage, p->zbin_over_quant,
                    p->zbin_mode_boost, p->act_zbin_adj, QUANT_ZBIN_MAX, p->planes, QUANT_PLANES);
    if (!p->job_qindex && (p->qindex < 0 || p->qindex > 127)) return fail(c, -2, "%s: qindex %d (0..127)", who, p->qindex);
    if (p->job_qindex)
        for (int i = 0; i < n; i++)
            if (p->job_qindex[i] > 127) return fail(c, -2, "%s: job_qindex[%d] = %d (0..127)", who, i, p->job_qindex[i]);
    if (stats && !p->planes) return fail(c, -2, "%s: stats without planes", who);
    const size_t grid = (size_t)c->dg.mb_cols * c->dg.mb_rows;
    const struct { const void *p; size_t stride, size, align; const char *name; } t[5] = {
        {coef, coef_stride, vp8hip_quant_coef_size(c), 16, "coef"}, {eob, eob_stride, vp8hip_quant_eob_size(c), 4, "eob"},
        {stats, stats_stride, vp8hip_quant_stats_size(c, p), 4, "stats"}, {rec, rec_stride, vp8hip_i420_size(c->width, c->height), 1, "rec"},
        {mv, mv_stride, 4 * grid, 2, "mv"}};
    for (const auto &a : t)
        if (a.p)
            if (int rc = vp8hip_check_named_dst(c, who, a.name, a.p, a.stride, a.size, a.align, n)) return rc;
    for (int a = 0; a < 4; a++)                              // the outputs against each other and against mv
        for (int b = a + 1; b < 5; b++)
            if (t[a].p && t[b].p && vp8hip_spans_overlap(t[a].p, t[a].stride, n, t[b].p, t[b].stride, n))
                return fail(c, -2, "%s: %s and %s overlap", who, t[a].name, t[b].name);
    HIPCHK(c, hipSetDevice(c->device));

    QuantLaunch L;
    memset(&L, 0, sizeof(L));
    vp8hip_frame_planes(c, L);
    L.filter = p->filter;
    L.fast = p->quantizer == VP8HIP_QUANT_FAST;
    L.levels = p->stage == VP8HIP_COEF_LEVELS;
    L.planes = stats ? p->planes : 0;
    L.mv = mv != nullptr;
    L.coef = coef != nullptr;
    L.eob = eob != nullptr;
    L.rec = rec != nullptr;
    for (int i0 = 0; i0 < n;) {
        int m = 0, tables = 0, qof[QUANT_MAX_TABLES];
        for (; i0 + m < n && m < QUANT_MAX_JOBS; m++) {
            const int q = p->job_qindex ? p->job_qindex[i0 + m] : p->qindex;
            int k = 0;
            while (k < tables && qof[k] != q) k++;
            if (k == tables) {
                if (tables == QUANT_MAX_TABLES) break;
                qof[tables] = q;
                vp8hip_quant_staged_table(L.t[tables++], q, p);
            }
            L.j[m] = QuantJob{vp8hip_frame_ref(c, jobs[i0 + m].fb), vp8hip_frame_ref(c, jobs[i0 + m].ref_fb), k};
        }
        auto at = [i0](const void *ptr, size_t stride) { return ptr ? (uint8_t *)ptr + stride * (size_t)i0 : nullptr; };
        hipLaunchKernelGGL(vp8_quant_frames_kernel, dim3((unsigned)grid, (unsigned)m), dim3(QUANT_THREADS), 0, c->stream, (const uint8_t *)c->fb_block,
                           c->fb_stride, (const uint8_t *)c->tile_block, c->tile_frame, (const uint8_t *)at(mv, mv_stride), mv_stride,
                           at(coef, coef_stride), coef_stride, at(eob, eob_stride), eob_stride, at(stats, stats_stride), stats_stride,
                           at(rec, rec_stride), rec_stride, L);
        HIPCHK(c, hipGetLastError());
        i0 += m;
    }
    return 0;
}
