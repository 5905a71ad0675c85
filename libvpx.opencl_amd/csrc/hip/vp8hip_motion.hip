// vp8hip_frames_motion_async (include/vp8hip.h): per macroblock of a picture pair the whole-pixel vector vp8_full_search_sad_c finds
// and what that match costs, as an int16 vector tensor and uint32 planes on the macroblock grid in the caller's device memory.
// The plan and the checks are made here, once per call; the kernel is in vp8_motion.hip.  Everything it reads is in the frame
// buffers as they lie (either form, nothing converted), in the caller's centre tensor or comes with the launch -- the cost table
// included --: nothing is allocated on the device, copied or synchronised.
#include "vp8hip_ctx.hip.h"

extern "C" __global__ void vp8_motion_frames_kernel(const uint8_t *raster, size_t fb_stride, const uint8_t *tiles, size_t tile_frame, const uint8_t *centre,
                                                    size_t centre_stride, uint8_t *mv, size_t mv_stride, uint8_t *stats, size_t stats_stride,
                                                    MotionLaunch L);

#define MOTION_PLANES (VP8HIP_MOTION_SAD | VP8HIP_MOTION_SAD0 | VP8HIP_MOTION_SSE | VP8HIP_MOTION_VAR | VP8HIP_MOTION_SRCVAR)
#define MOTION_LDS_FIXED (8 + 64 + 2 * (2 * MOTION_MAX_D + 2))      // dwords in front of the window (vp8_motion.hip: MOTION_LDS_WINDOW)

// what the call refuses on p alone
static bool motion_params_ok(const vp8hip_motion *p)
{
    return p && p->distance >= 1 && p->distance <= MOTION_MAX_D && !(p->planes & ~(unsigned)MOTION_PLANES) && p->sad_per_bit >= 0 && p->sad_per_bit <= 255;
}

extern "C" size_t vp8hip_motion_mv_size(const vp8hip_ctx *c)
{
    return c && c->width ? (size_t)4 * c->dg.mb_cols * c->dg.mb_rows : 0;
}

extern "C" size_t vp8hip_motion_stats_size(const vp8hip_ctx *c, const vp8hip_motion *p)
{
    if (!c || !c->width || !motion_params_ok(p) || !p->planes) return 0;
    return (size_t)4 * __builtin_popcount(p->planes) * c->dg.mb_cols * c->dg.mb_rows;
}

extern "C" int vp8hip_frames_motion_async(vp8hip_ctx *c, const vp8hip_hist_job *jobs, int n, const vp8hip_motion *p, const void *centre,
                                          size_t centre_stride, void *mv, size_t mv_stride, void *stats, size_t stats_stride)
{
    const char *who = "vp8hip_frames_motion_async";
    if (!c || !jobs || n < 1 || !p || (!mv && !stats) || !c->width || c->fb.empty()) return fail(c, -2, "%s: bad arguments", who);
    if (int rc = vp8hip_check_pairs(c, who, jobs, n, false)) return rc;
    if (!motion_params_ok(p))
        return fail(c, -2, "%s: distance %d (1..%d), sad_per_bit %d (0..255), planes 0x%x (of 0x%x)", who, p->distance, MOTION_MAX_D, p->sad_per_bit,
                    p->planes, MOTION_PLANES);
    if (stats && !p->planes) return fail(c, -2, "%s: stats without planes", who);
    const int d = p->distance;
    MotionLaunch L;
    memset(&L, 0, sizeof(L) - sizeof(L.j));
    if (p->cost && p->sad_per_bit) {
        for (int k = 0; k < 2; k++)
            for (int i = 0; i <= 2 * d; i++) {
                const int32_t v = p->cost[k * (2 * d + 1) + i];
                if (v < 0 || v > 65535) return fail(c, -2, "%s: cost[%d][%d] = %d (0..65535)", who, k, i, v);
                L.cost[k][i] = (unsigned short)v;
            }
        L.spb = p->sad_per_bit;
    }
    // the vectors are (candidate << 3) in int16: with a centre tensor a candidate reaches 16 macroblocks past the picture's far side
    if (centre && (c->dg.mb_cols > 255 || c->dg.mb_rows > 255))
        return fail(c, -2, "%s: a centre tensor on more than 255 macroblocks a side", who);
    const size_t mv_size = vp8hip_motion_mv_size(c), stats_size = vp8hip_motion_stats_size(c, p);
    if (mv)
        if (int rc = vp8hip_check_named_dst(c, who, "mv", mv, mv_stride, mv_size, 2, n)) return rc;
    if (stats)
        if (int rc = vp8hip_check_named_dst(c, who, "stats", stats, stats_stride, stats_size, 4, n)) return rc;
    if (centre)
        if (int rc = vp8hip_check_named_dst(c, who, "centre", centre, centre_stride, mv_size, 2, n)) return rc;
    if (mv && stats && vp8hip_spans_overlap(mv, mv_stride, n, stats, stats_stride, n)) return fail(c, -2, "%s: mv and stats overlap", who);
    if (mv && centre && vp8hip_spans_overlap(mv, mv_stride, n, centre, centre_stride, n)) return fail(c, -2, "%s: mv and centre overlap", who);
    if (stats && centre && vp8hip_spans_overlap(stats, stats_stride, n, centre, centre_stride, n))
        return fail(c, -2, "%s: stats and centre overlap", who);
    HIPCHK(c, hipSetDevice(c->device));

    vp8hip_frame_planes(c, L);
    L.d = d;
    L.nq = (2 * d + 3) / 4;
    L.groups = (2 * d + MOTION_ROWS - 1) / MOTION_ROWS;
    L.rows = MOTION_ROWS * L.groups + 15;
    // a half-wave spans 32 / nq rows of items, MOTION_ROWS * pitch dwords apart: pad the pitch until they start nq banks apart
    L.pitch = L.nq + 4;
    if (L.nq >= 4 && L.nq < 32 && 32 % L.nq == 0)
        while ((MOTION_ROWS * L.pitch) % L.nq || !((MOTION_ROWS * L.pitch / L.nq) & 1)) L.pitch++;
    L.planes = stats ? p->planes : 0;
    L.mv = mv != nullptr;
    L.centre = centre != nullptr;
    const int items = L.groups * L.nq;
    const unsigned threads = items > 192 ? 256u : (unsigned)((items + 63) / 64 * 64);
    const size_t lds = (size_t)(MOTION_LDS_FIXED + L.rows * L.pitch) * 4;
    for (int i0 = 0; i0 < n; i0 += MOTION_MAX_JOBS) {
        const int m = n - i0 < MOTION_MAX_JOBS ? n - i0 : MOTION_MAX_JOBS;
        for (int k = 0; k < m; k++) {
            L.j[k].fb = vp8hip_frame_ref(c, jobs[i0 + k].fb);
            L.j[k].ref = vp8hip_frame_ref(c, jobs[i0 + k].ref_fb);
        }
        const uint8_t *dc = centre ? (const uint8_t *)centre + centre_stride * (size_t)i0 : nullptr;
        uint8_t *dv = mv ? (uint8_t *)mv + mv_stride * (size_t)i0 : nullptr;
        uint8_t *ds = stats ? (uint8_t *)stats + stats_stride * (size_t)i0 : nullptr;
        hipLaunchKernelGGL(vp8_motion_frames_kernel, dim3((unsigned)(L.mb_cols * L.mb_rows), (unsigned)m), dim3(threads), lds, c->stream,
                           (const uint8_t *)c->fb_block, c->fb_stride, (const uint8_t *)c->tile_block, c->tile_frame, dc, centre_stride, dv, mv_stride,
                           ds, stats_stride, L);
        HIPCHK(c, hipGetLastError());
    }
    return 0;
}
