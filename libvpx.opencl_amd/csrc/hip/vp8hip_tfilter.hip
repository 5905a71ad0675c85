// vp8hip_frames_tfilter_async (include/vp8hip.h): the reference's motion-compensated temporal filter (vp8/encoder/temporal_filter.c)
// of a centre picture over up to fifteen source pictures, each with the vectors and the errors vp8hip_frames_subpel_async left for
// the pair, as a packed I420 picture and a per-pixel count in the caller's device memory.  The plan and the checks are made here,
// once per call; the kernel is in vp8_tfilter.hip.  Everything it reads is in the frame buffers as they lie (either form, nothing
// converted), in the caller's tensors, or comes with the launch: no device memory is added.  A launch carries its jobs and a copy
// of each job's sources in its arguments (TfilterLaunch), so a call of many jobs is cut where either array is full.
#include "vp8hip_ctx.hip.h"

extern "C" __global__ void vp8_tfilter_frames_kernel(const uint8_t *raster, size_t fb_stride, const uint8_t *tiles, size_t tile_frame, const uint8_t *mv,
                                                     size_t mv_stride, const uint8_t *err, size_t err_stride, uint8_t *dst, size_t dst_stride,
                                                     uint8_t *cnt, size_t cnt_stride, TfilterLaunch L);

extern "C" size_t vp8hip_tfilter_count_size(const vp8hip_ctx *c)
{
    return c && c->width ? 2 * vp8hip_i420_size(c->width, c->height) : 0;
}

extern "C" int vp8hip_frames_tfilter_async(vp8hip_ctx *c, const vp8hip_tfilter_job *jobs, int n, const vp8hip_hist_job *pairs, int npairs,
                                           const vp8hip_tfilter *p, const void *mv, size_t mv_stride, const void *err, size_t err_stride, void *dst,
                                           size_t dst_stride, void *cnt, size_t cnt_stride)
{
    const char *who = "vp8hip_frames_tfilter_async";
    if (!c || !jobs || n < 1 || !pairs || npairs < 1 || !p || (!dst && !cnt) || !c->width || c->fb.empty()) return fail(c, -2, "%s: bad arguments", who);
    if (int rc = vp8hip_check_pairs(c, who, pairs, npairs, false)) return rc;
    for (int i = 0; i < n; i++) {
        const vp8hip_tfilter_job &j = jobs[i];
        if (int rc = vp8hip_check_fbs(c, who, &j.fb, 1)) return rc;
        if (j.count < 1 || j.count > TFILTER_MAX_COUNT || j.first < 0 || j.first > npairs - j.count)
            return fail(c, -2, "%s: job %d takes pairs %d .. + %d (1..%d of them, inside the list's %d)", who, i, j.first, j.count, TFILTER_MAX_COUNT,
                        npairs);
        for (int k = j.first; k < j.first + j.count; k++)
            if (pairs[k].fb != j.fb) return fail(c, -2, "%s: pair %d is of frame buffer %d, job %d filters %d", who, k, pairs[k].fb, i, j.fb);
    }
    if (p->strength < 0 || p->strength > 6 || (p->filter != VP8HIP_TFILTER_SIXTAP && p->filter != VP8HIP_TFILTER_BILINEAR) ||
        p->thresh_high < p->thresh_low)
        return fail(c, -2, "%s: strength %d (0..6), filter %d (0, 1), thresholds %u, %u (low <= high)", who, p->strength, p->filter, p->thresh_low,
                    p->thresh_high);
    const size_t pic = vp8hip_i420_size(c->width, c->height), grid = (size_t)c->dg.mb_cols * c->dg.mb_rows;
    if (dst)
        if (int rc = vp8hip_check_named_dst(c, who, "dst", dst, dst_stride, pic, 1, n)) return rc;
    if (cnt)
        if (int rc = vp8hip_check_named_dst(c, who, "cnt", cnt, cnt_stride, 2 * pic, 2, n)) return rc;
    if (mv)
        if (int rc = vp8hip_check_named_dst(c, who, "mv", mv, mv_stride, 4 * grid, 2, npairs)) return rc;
    if (err)
        if (int rc = vp8hip_check_named_dst(c, who, "err", err, err_stride, 4 * grid, 4, npairs)) return rc;
    if (dst && cnt && vp8hip_spans_overlap(dst, dst_stride, n, cnt, cnt_stride, n)) return fail(c, -2, "%s: dst and cnt overlap", who);
    const struct { const void *p; size_t stride; const char *name; } in[2] = {{mv, mv_stride, "mv"}, {err, err_stride, "err"}};
    for (const auto &t : in) {
        if (!t.p) continue;
        if (dst && vp8hip_spans_overlap(dst, dst_stride, n, t.p, t.stride, npairs)) return fail(c, -2, "%s: dst and %s overlap", who, t.name);
        if (cnt && vp8hip_spans_overlap(cnt, cnt_stride, n, t.p, t.stride, npairs)) return fail(c, -2, "%s: cnt and %s overlap", who, t.name);
    }
    HIPCHK(c, hipSetDevice(c->device));

    TfilterLaunch L;
    memset(&L, 0, sizeof(L));
    vp8hip_frame_planes(c, L);
    L.strength = p->strength;
    L.filter = p->filter;
    L.lo = p->thresh_low;
    L.hi = p->thresh_high;
    L.mv = mv != nullptr;
    L.err = err != nullptr;
    L.dst = dst != nullptr;
    L.cnt = cnt != nullptr;
    for (int i0 = 0; i0 < n;) {
        int m = 0, refs = 0;
        for (; i0 + m < n && m < TFILTER_MAX_JOBS && refs + jobs[i0 + m].count <= TFILTER_MAX_REFS; m++) {
            const vp8hip_tfilter_job &j = jobs[i0 + m];
            L.j[m] = TfilterJob{vp8hip_frame_ref(c, j.fb), j.first, j.count, refs};
            for (int k = 0; k < j.count; k++) L.ref[refs++] = vp8hip_frame_ref(c, pairs[j.first + k].ref_fb);
        }
        uint8_t *dp = dst ? (uint8_t *)dst + dst_stride * (size_t)i0 : nullptr;
        uint8_t *dc = cnt ? (uint8_t *)cnt + cnt_stride * (size_t)i0 : nullptr;
        hipLaunchKernelGGL(vp8_tfilter_frames_kernel, dim3((unsigned)grid, (unsigned)m), dim3(TFILTER_THREADS), 0, c->stream,
                           (const uint8_t *)c->fb_block, c->fb_stride, (const uint8_t *)c->tile_block, c->tile_frame, (const uint8_t *)mv, mv_stride,
                           (const uint8_t *)err, err_stride, dp, dst_stride, dc, cnt_stride, L);
        HIPCHK(c, hipGetLastError());
        i0 += m;
    }
    return 0;
}
