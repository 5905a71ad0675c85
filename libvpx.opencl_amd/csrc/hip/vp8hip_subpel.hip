// vp8hip_frames_subpel_async (include/vp8hip.h): per macroblock of a picture pair the sub-pixel vector vp8_find_best_sub_pixel_step
// (or, at precision 2, vp8_find_best_half_pixel_step) finds around a whole-pixel start, and what that match costs, as an int16
// vector tensor and uint32 planes on the macroblock grid in the caller's device memory.  The plan and the checks are made here, once
// per call; the kernel is in vp8_subpel.hip.  Everything it reads is in the frame buffers as they lie (either form, nothing
// converted), in the caller's start and reference tensors, or comes with the launch -- except the cost table, up to 8188 bytes: that
// goes to a copy the context owns (vp8hip_ctx::d_subpel_cost, 8 KB, made with the first call that has a table: the call's one
// allocation), in pieces that ride in the arguments of small launches ahead of the kernel.  So the caller's table is read at the
// call and never later, nothing is synchronised, and calls queued back to back with different tables each read their own: the
// stream orders piece, kernel, piece, kernel.
#include "vp8hip_ctx.hip.h"

extern "C" __global__ void vp8_subpel_frames_kernel(const uint8_t *raster, size_t fb_stride, const uint8_t *tiles, size_t tile_frame, const uint8_t *start,
                                                    size_t start_stride, const uint8_t *ref, size_t ref_stride, uint8_t *mv, size_t mv_stride,
                                                    uint8_t *stats, size_t stats_stride, const unsigned short *cost, SubpelLaunch L);
extern "C" __global__ void vp8_subpel_table_kernel(unsigned short *dst, SubpelTablePiece P);

#define SUBPEL_PLANES (VP8HIP_SUBPEL_VAL | VP8HIP_SUBPEL_VAR | VP8HIP_SUBPEL_SSE | VP8HIP_SUBPEL_VAR0)
#define SUBPEL_MAX_EPB 16383

// what the call refuses on p alone (the table and its range apart: they count only where the table is read)
static bool subpel_params_ok(const vp8hip_subpel *p)
{
    return p && (p->precision == 2 || p->precision == 4) && !(p->planes & ~(unsigned)SUBPEL_PLANES) && p->error_per_bit >= 0 &&
           p->error_per_bit <= SUBPEL_MAX_EPB;
}

extern "C" size_t vp8hip_subpel_mv_size(const vp8hip_ctx *c)
{
    return c && c->width ? (size_t)4 * c->dg.mb_cols * c->dg.mb_rows : 0;
}

extern "C" size_t vp8hip_subpel_stats_size(const vp8hip_ctx *c, const vp8hip_subpel *p)
{
    if (!c || !c->width || !subpel_params_ok(p) || !p->planes) return 0;
    return (size_t)4 * __builtin_popcount(p->planes) * c->dg.mb_cols * c->dg.mb_rows;
}

extern "C" int vp8hip_frames_subpel_async(vp8hip_ctx *c, const vp8hip_hist_job *jobs, int n, const vp8hip_subpel *p, const void *start,
                                          size_t start_stride, const void *ref, size_t ref_stride, void *mv, size_t mv_stride, void *stats,
                                          size_t stats_stride)
{
    const char *who = "vp8hip_frames_subpel_async";
    if (!c || !jobs || n < 1 || !p || (!mv && !stats) || !c->width || c->fb.empty()) return fail(c, -2, "%s: bad arguments", who);
    if (int rc = vp8hip_check_pairs(c, who, jobs, n, false)) return rc;
    if (!subpel_params_ok(p))
        return fail(c, -2, "%s: precision %d (2 or 4), error_per_bit %d (0..%d), planes 0x%x (of 0x%x)", who, p->precision, p->error_per_bit,
                    SUBPEL_MAX_EPB, p->planes, SUBPEL_PLANES);
    if (stats && !p->planes) return fail(c, -2, "%s: stats without planes", who);
    const bool costed = p->cost && p->error_per_bit;
    const int R = p->cost_range;
    if (costed) {
        if (R < 1 || R > SUBPEL_MAX_RANGE) return fail(c, -2, "%s: cost_range %d (1..%d)", who, R, SUBPEL_MAX_RANGE);
        for (int k = 0; k < 2; k++)
            for (int i = 0; i <= 2 * R; i++) {
                const int32_t v = p->cost[k * (2 * R + 1) + i];
                if (v < 0 || v > 65535) return fail(c, -2, "%s: cost[%d][%d] = %d (0..65535)", who, k, i, v);
            }
    }
    // the vectors are 8 * start + a step in int16: a clamped start reaches 16 macroblocks past the picture's far side
    if (start && (c->dg.mb_cols > 255 || c->dg.mb_rows > 255)) return fail(c, -2, "%s: a start tensor on more than 255 macroblocks a side", who);
    const size_t mv_size = vp8hip_subpel_mv_size(c), stats_size = vp8hip_subpel_stats_size(c, p);
    if (mv)
        if (int rc = vp8hip_check_named_dst(c, who, "mv", mv, mv_stride, mv_size, 2, n)) return rc;
    if (stats)
        if (int rc = vp8hip_check_named_dst(c, who, "stats", stats, stats_stride, stats_size, 4, n)) return rc;
    if (start)
        if (int rc = vp8hip_check_named_dst(c, who, "start", start, start_stride, mv_size, 2, n)) return rc;
    if (ref)
        if (int rc = vp8hip_check_named_dst(c, who, "ref", ref, ref_stride, mv_size, 2, n)) return rc;
    if (mv && stats && vp8hip_spans_overlap(mv, mv_stride, n, stats, stats_stride, n)) return fail(c, -2, "%s: mv and stats overlap", who);
    const struct { const void *p; size_t stride; const char *name; } in[2] = {{start, start_stride, "start"}, {ref, ref_stride, "ref"}};
    for (const auto &t : in) {
        if (!t.p) continue;
        if (mv && vp8hip_spans_overlap(mv, mv_stride, n, t.p, t.stride, n)) return fail(c, -2, "%s: mv and %s overlap", who, t.name);
        if (stats && vp8hip_spans_overlap(stats, stats_stride, n, t.p, t.stride, n)) return fail(c, -2, "%s: stats and %s overlap", who, t.name);
    }
    HIPCHK(c, hipSetDevice(c->device));

    if (costed) {
        if (c->d_subpel_cost.grow(SUBPEL_TABLE_ENTRIES) != hipSuccess) return fail(c, -1, "%s: no device memory for the cost table", who);
        const int entries = 2 * (2 * R + 1);
        SubpelTablePiece P;
        for (int first = 0; first < entries; first += SUBPEL_TABLE_PIECE) {
            P.first = first;
            P.n = entries - first < SUBPEL_TABLE_PIECE ? entries - first : SUBPEL_TABLE_PIECE;
            for (int i = 0; i < P.n; i++) P.v[i] = (unsigned short)p->cost[first + i];
            hipLaunchKernelGGL(vp8_subpel_table_kernel, dim3(1), dim3(256), 0, c->stream, c->d_subpel_cost.p, P);
            HIPCHK(c, hipGetLastError());
        }
    }

    SubpelLaunch L;
    memset(&L, 0, sizeof(L) - sizeof(L.j));
    vp8hip_frame_planes(c, L);
    L.precision = p->precision;
    L.epb = costed ? p->error_per_bit : 0;
    L.R = costed ? R : 0;
    L.planes = stats ? p->planes : 0;
    L.mv = mv != nullptr;
    L.start = start != nullptr;
    L.ref = costed && ref != nullptr;
    const int nmb = L.mb_cols * L.mb_rows;
    for (int i0 = 0; i0 < n; i0 += SUBPEL_MAX_JOBS) {
        const int m = n - i0 < SUBPEL_MAX_JOBS ? n - i0 : SUBPEL_MAX_JOBS;
        for (int k = 0; k < m; k++) {
            L.j[k].fb = vp8hip_frame_ref(c, jobs[i0 + k].fb);
            L.j[k].ref = vp8hip_frame_ref(c, jobs[i0 + k].ref_fb);
        }
        const uint8_t *ds0 = start ? (const uint8_t *)start + start_stride * (size_t)i0 : nullptr;
        const uint8_t *dr = L.ref ? (const uint8_t *)ref + ref_stride * (size_t)i0 : nullptr;
        uint8_t *dv = mv ? (uint8_t *)mv + mv_stride * (size_t)i0 : nullptr;
        uint8_t *ds = stats ? (uint8_t *)stats + stats_stride * (size_t)i0 : nullptr;
        hipLaunchKernelGGL(vp8_subpel_frames_kernel, dim3((unsigned)((nmb + SUBPEL_WAVES - 1) / SUBPEL_WAVES), (unsigned)m), dim3(64 * SUBPEL_WAVES), 0,
                           c->stream, (const uint8_t *)c->fb_block, c->fb_stride, (const uint8_t *)c->tile_block, c->tile_frame, ds0, start_stride, dr,
                           ref_stride, dv, mv_stride, ds, stats_stride, (const unsigned short *)c->d_subpel_cost.p, L);
        HIPCHK(c, hipGetLastError());
    }
    return 0;
}
