// vp8hip_frames_intra_async, vp8hip_intra_costs and vp8hip_intra_rd (include/vp8hip.h): the reference's intra mode decision and
// encode of every macroblock of a key frame -- vp8_pick_intra_mode, then the body of vp8cx_encode_intra_macro_block -- as level
// records, eobs, modes, decision figures and a packed I420 reconstruction in the caller's device memory.  The plan and the checks
// are made here, once per call; the kernel is in vp8_intra_enc.hip: one workgroup a job.  Everything it reads is in the frame
// buffers as they lie or comes with the launch (IntraLaunch: the jobs, one quantiser table per distinct qindex among them, the mode
// costs), so a call of many jobs is cut where either array is full; no device memory is added.
#include "vp8hip_ctx.hip.h"

extern "C" __global__ void vp8_intra_enc_kernel(const uint8_t *raster, size_t fb_stride, const uint8_t *tiles, size_t tile_frame, uint8_t *coef,
                                                size_t coef_stride, uint8_t *eobs, size_t eob_stride, uint8_t *stats, size_t stats_stride, uint8_t *rec,
                                                size_t rec_stride, uint8_t *modes, size_t modes_stride, IntraLaunch L);

namespace intra_tables {
#include "../host/vp8_enc_tables.c"
static const uint8_t kf_bmode_probs[900] = {
#include "../host/vp8_kf_bmode_probs.inc"
};
}

#define INTRA_PLANES (VP8HIP_INTRA_RD16 | VP8HIP_INTRA_RD4 | VP8HIP_INTRA_RATE | VP8HIP_INTRA_EOBS | VP8HIP_INTRA_RECSSE)
// the launch's arguments must fit the 4 KiB a kernel takes: the struct and the fourteen scalars before it
static_assert(sizeof(IntraLaunch) + 14 * 8 <= 4096 && INTRA_MAX_TABLES <= 4, "");

// vp8_cost_tokens for one leaf: its path as (bit, probability index) pairs, ended by index -1
struct IntraPath { signed char bit, idx; };
static int path_cost(const IntraPath *path, const uint8_t *probs)
{
    int c = 0;
    for (; path->idx >= 0; path++) c += intra_tables::vp8t_prob_cost[path->bit ? 255 - probs[path->idx] : probs[path->idx]];
    return c;
}

extern "C" int vp8hip_intra_costs(vp8hip_intra_cost *out)
{
    // vp8_kf_ymode_tree over vp8_kf_ymode_prob: B_PRED "0", DC "100", V "101", H "110", TM "111"
    static const uint8_t ymode_prob[4] = {145, 156, 163, 128};
    static const IntraPath ymode[5][4] = {{{1, 0}, {0, 1}, {0, 2}, {0, -1}}, {{1, 0}, {0, 1}, {1, 2}, {0, -1}}, {{1, 0}, {1, 1}, {0, 3}, {0, -1}},
                                          {{1, 0}, {1, 1}, {1, 3}, {0, -1}}, {{0, 0}, {0, -1}}};
    // vp8_bmode_tree: B_DC "0", B_TM "10", B_VE "110", B_HE "11100", B_LD "11110", B_RD "111010", B_VR "111011", B_VL "111110",
    // B_HD "1111110", B_HU "1111111"
    static const IntraPath bmode[10][8] = {
        {{0, 0}, {0, -1}},
        {{1, 0}, {0, 1}, {0, -1}},
        {{1, 0}, {1, 1}, {0, 2}, {0, -1}},
        {{1, 0}, {1, 1}, {1, 2}, {0, 3}, {0, 4}, {0, -1}},
        {{1, 0}, {1, 1}, {1, 2}, {1, 3}, {0, 6}, {0, -1}},
        {{1, 0}, {1, 1}, {1, 2}, {0, 3}, {1, 4}, {0, 5}, {0, -1}},
        {{1, 0}, {1, 1}, {1, 2}, {0, 3}, {1, 4}, {1, 5}, {0, -1}},
        {{1, 0}, {1, 1}, {1, 2}, {1, 3}, {1, 6}, {0, 7}, {0, -1}},
        {{1, 0}, {1, 1}, {1, 2}, {1, 3}, {1, 6}, {1, 7}, {0, 8}, {0, -1}},
        {{1, 0}, {1, 1}, {1, 2}, {1, 3}, {1, 6}, {1, 7}, {1, 8}, {0, -1}}};
    if (!out) return -2;
    for (int m = 0; m < 5; m++) out->mbmode_cost[m] = path_cost(ymode[m], ymode_prob);
    for (int a = 0; a < 10; a++)
        for (int l = 0; l < 10; l++)
            for (int m = 0; m < 10; m++) out->bmode_cost[a][l][m] = path_cost(bmode[m], intra_tables::kf_bmode_probs + 9 * (10 * a + l));
    return 0;
}

extern "C" int vp8hip_intra_rd(int qindex, int y1dc_delta, int zbin_over_quant, int *rdmult, int *rddiv)
{
    static const unsigned short dc_q[128] = { VP8_DC_Q_VALUES };
    if (!rdmult || !rddiv || qindex < 0 || qindex > 127 || y1dc_delta < -15 || y1dc_delta > 15) return -2;
    int qi = qindex + y1dc_delta;
    qi = qi < 0 ? 0 : qi > 127 ? 127 : qi;
    const int Qvalue = dc_q[qi];
    // vp8_initialize_rd_consts, as written there
    double capped_q = (Qvalue < 160) ? (double)Qvalue : 160.0;
    double rdconst = 2.70;
    int m = (int)(rdconst * (capped_q * capped_q));
    if (zbin_over_quant > 0) {
        double oq_factor = 1.0 + ((double)0.0015625 * zbin_over_quant);
        double modq = (int)((double)capped_q * oq_factor);
        m = (int)(rdconst * (modq * modq));
    }
    if (m > 1000) {
        *rddiv = 1;
        m /= 100;
    } else
        *rddiv = 100;
    *rdmult = m;
    return 0;
}

extern "C" size_t vp8hip_intra_modes_size(const vp8hip_ctx *c) { return c && c->width ? (size_t)32 * c->dg.mb_cols * c->dg.mb_rows : 0; }
extern "C" size_t vp8hip_intra_stats_size(const vp8hip_ctx *c, const vp8hip_intra *p)
{
    if (!c || !c->width || !p || !p->planes || (p->planes & ~(unsigned)INTRA_PLANES)) return 0;
    return (size_t)4 * __builtin_popcount(p->planes) * c->dg.mb_cols * c->dg.mb_rows;
}

extern "C" int vp8hip_frames_intra_async(vp8hip_ctx *c, const int *fb, int n, const vp8hip_intra *p, void *coef, size_t coef_stride, void *eob,
                                         size_t eob_stride, void *stats, size_t stats_stride, void *rec, size_t rec_stride, void *modes,
                                         size_t modes_stride)
{
    const char *who = "vp8hip_frames_intra_async";
    if (!c || !fb || n < 1 || !p || (!coef && !eob && !stats && !rec && !modes) || !c->width || c->fb.empty())
        return fail(c, -2, "%s: bad arguments", who);
    if (int rc = vp8hip_check_fbs(c, who, fb, n)) return rc;
    const vp8hip_quant *q = &p->q;
    if (!vp8hip_quantiser_ok(q))
        return fail(c, -2, "%s: deltas %d %d %d %d %d (-15..15), quantizer %d, stage %d (0, 1), zero-bin terms %d %d %d (+-%d)", who, q->delta[0],
                    q->delta[1], q->delta[2], q->delta[3], q->delta[4], q->quantizer, q->stage, q->zbin_over_quant, q->zbin_mode_boost,
                    q->act_zbin_adj, QUANT_ZBIN_MAX);
    if (!q->job_qindex && (q->qindex < 0 || q->qindex > 127)) return fail(c, -2, "%s: qindex %d (0..127)", who, q->qindex);
    if (q->job_qindex)
        for (int i = 0; i < n; i++)
            if (q->job_qindex[i] > 127) return fail(c, -2, "%s: job_qindex[%d] = %d (0..127)", who, i, q->job_qindex[i]);
    if (p->rdmult < 0 || p->rdmult > 1000 || p->rddiv < 1 || p->rddiv > 100 || p->bmode_last < 0 || p->bmode_last > 9 ||
        (p->flags & ~(unsigned)VP8HIP_INTRA_NO_BPRED) || (p->planes & ~(unsigned)INTRA_PLANES))
        return fail(c, -2, "%s: rdmult %d (0..1000), rddiv %d (1..100), bmode_last %d (0..9), flags 0x%x (of 0x%x), planes 0x%x (of 0x%x)", who,
                    p->rdmult, p->rddiv, p->bmode_last, p->flags, VP8HIP_INTRA_NO_BPRED, p->planes, INTRA_PLANES);
    for (int i = 0; i < 5; i++)
        if (p->cost.mbmode_cost[i] < 0 || p->cost.mbmode_cost[i] > 65535) return fail(c, -2, "%s: mbmode_cost[%d] = %d (0..65535)", who, i, p->cost.mbmode_cost[i]);
    for (int i = 0; i < 1000; i++)
        if ((&p->cost.bmode_cost[0][0][0])[i] < 0 || (&p->cost.bmode_cost[0][0][0])[i] > 65535)
            return fail(c, -2, "%s: bmode_cost[%d][%d][%d] = %d (0..65535)", who, i / 100, i / 10 % 10, i % 10, (&p->cost.bmode_cost[0][0][0])[i]);
    if (stats && !p->planes) return fail(c, -2, "%s: stats without planes", who);
    const struct { const void *p; size_t stride, size, align; const char *name; } t[5] = {
        {coef, coef_stride, vp8hip_quant_coef_size(c), 16, "coef"}, {eob, eob_stride, vp8hip_quant_eob_size(c), 4, "eob"},
        {stats, stats_stride, vp8hip_intra_stats_size(c, p), 4, "stats"}, {rec, rec_stride, vp8hip_i420_size(c->width, c->height), 1, "rec"},
        {modes, modes_stride, vp8hip_intra_modes_size(c), 4, "modes"}};
    for (const auto &a : t)
        if (a.p)
            if (int rc = vp8hip_check_named_dst(c, who, a.name, a.p, a.stride, a.size, a.align, n)) return rc;
    for (int a = 0; a < 4; a++)
        for (int b = a + 1; b < 5; b++)
            if (t[a].p && t[b].p && vp8hip_spans_overlap(t[a].p, t[a].stride, n, t[b].p, t[b].stride, n))
                return fail(c, -2, "%s: %s and %s overlap", who, t[a].name, t[b].name);
    HIPCHK(c, hipSetDevice(c->device));

    IntraLaunch L;
    memset(&L, 0, sizeof(L));
    vp8hip_frame_planes(c, L);
    L.fast = q->quantizer == VP8HIP_QUANT_FAST;
    L.levels = q->stage == VP8HIP_COEF_LEVELS;
    L.planes = stats ? p->planes : 0;
    L.coef = coef != nullptr;
    L.eob = eob != nullptr;
    L.rec = rec != nullptr;
    L.modes = modes != nullptr;
    L.rdmult = p->rdmult;
    L.rddiv = p->rddiv;
    L.bmode_last = p->bmode_last;
    L.no_bpred = (p->flags & VP8HIP_INTRA_NO_BPRED) != 0;
    for (int i = 0; i < 5; i++) L.mbmode_cost[i] = (unsigned short)p->cost.mbmode_cost[i];
    for (int i = 0; i < 1000; i++) L.bmode_cost[i] = (unsigned short)(&p->cost.bmode_cost[0][0][0])[i];
    // the line the last row of a band leaves for the next band: only where there is a next band (at most 1024 columns: 36 KB,
    // with the kernel's 27 KB of static LDS inside the 64 KB a workgroup has without asking for more)
    const size_t dyn = L.mb_rows > INTRA_BAND ? (size_t)L.mb_cols * INTRA_LINE_WORDS * 4 : 0;
    for (int i0 = 0; i0 < n;) {
        int m = 0, tables = 0, qof[INTRA_MAX_TABLES];
        for (; i0 + m < n && m < INTRA_MAX_JOBS; m++) {
            const int qi = q->job_qindex ? q->job_qindex[i0 + m] : q->qindex;
            int k = 0;
            while (k < tables && qof[k] != qi) k++;
            if (k == tables) {
                if (tables == INTRA_MAX_TABLES) break;
                qof[tables] = qi;
                vp8hip_quant_staged_table(L.t[tables++], qi, q);
            }
            L.j[m] = vp8hip_frame_ref(c, fb[i0 + m]) | k << 28;
        }
        auto at = [i0](void *ptr, size_t stride) { return ptr ? (uint8_t *)ptr + stride * (size_t)i0 : nullptr; };
        hipLaunchKernelGGL(vp8_intra_enc_kernel, dim3((unsigned)m), dim3(INTRA_THREADS), dyn, c->stream, (const uint8_t *)c->fb_block, c->fb_stride,
                           (const uint8_t *)c->tile_block, c->tile_frame, at(coef, coef_stride), coef_stride, at(eob, eob_stride), eob_stride,
                           at(stats, stats_stride), stats_stride, at(rec, rec_stride), rec_stride, at(modes, modes_stride), modes_stride, L);
        HIPCHK(c, hipGetLastError());
        i0 += m;
    }
    return 0;
}
