// vp8hip_frames_ssim_async (include/vp8hip.h): the structural similarity of picture pairs, vp8_ssim2's windows over the display-size
// planes of two frame buffers, as Q32 totals [planes][2] of int64 and as a map of the window values, in the caller's device memory.
// The plan and the checks are made here, once per call; the kernels are in vp8_ssim.hip.  Everything they read is in the frame
// buffers as they lie (either form, nothing converted) or comes with the launch: nothing is allocated on the device, copied or
// synchronised.
#include "vp8hip_ctx.hip.h"

extern "C" __global__ void vp8_ssim_fill_kernel(uint8_t *dst, size_t dst_stride, SsimFill F);
extern "C" __global__ void vp8_ssim_frames_kernel(const uint8_t *raster, size_t fb_stride, const uint8_t *tiles, size_t tile_frame, uint8_t *scores,
                                                  size_t scores_stride, uint8_t *map, size_t map_stride, SsimLaunch L);

#define SSIM_CHIP_WGS 2048                      // workgroups a call aims at: calls of fewer jobs share a job's pieces among several

extern "C" int vp8hip_ssim_windows(int w, int h, int *nwx, int *nwy)
{
    const bool ok = w >= 1 && h >= 1 && w <= VP8HIP_MAX_OUT_SIZE && h <= VP8HIP_MAX_OUT_SIZE;
    if (nwx) *nwx = ok && w > 8 ? (w - 5) / 4 : 0;
    if (nwy) *nwy = ok && h > 8 ? (h - 5) / 4 : 0;
    return ok ? 0 : -2;
}

extern "C" size_t vp8hip_ssim_scores_size(int planes_popcount)
{
    return planes_popcount >= 1 && planes_popcount <= 3 ? (size_t)planes_popcount * 16 : 0;
}

// the planes of `planes` on context c, their windows, pieces and places in a job's map; false for planes the call refuses
static bool ssim_planes(const vp8hip_ctx *c, unsigned planes, SsimLaunch &L, size_t &map_elems)
{
    if (!c || !c->width || !planes || (planes & ~VP8HIP_HIST_YUV)) return false;
    L.np = L.pieces = 0;
    map_elems = 0;
    for (int pl = 0; pl < 3; pl++) {
        if (!((planes >> pl) & 1u)) continue;
        SsimPlane &P = L.p[L.np++];
        P.pl = pl;
        (void)vp8hip_ssim_windows(pl ? (c->width + 1) >> 1 : c->width, pl ? (c->height + 1) >> 1 : c->height, &P.nwx, &P.nwy);
        if (!P.nwx || !P.nwy) P.nwx = P.nwy = 0;      // (a plane of no windows has no rows of none either)
        P.px = (P.nwx + SSIM_BAND_COLS - 1) / SSIM_BAND_COLS;
        P.first = L.pieces;
        P.map_off = (int)map_elems;                     // (at most 3 * 4095^2)
        L.pieces += P.px * ((P.nwy + SSIM_BAND_ROWS - 1) / SSIM_BAND_ROWS);
        map_elems += (size_t)P.nwx * (size_t)P.nwy;
    }
    return true;
}

// workgroups that share a job of `pieces` pieces, in a call of n jobs
static int ssim_share(int n, int pieces)
{
    int S = (SSIM_CHIP_WGS + n - 1) / n;
    if (S > pieces) S = pieces;
    return S < 1 ? 1 : S;
}

extern "C" size_t vp8hip_ssim_map_size(const vp8hip_ctx *c, const vp8hip_ssim *p)
{
    SsimLaunch L;
    size_t elems = 0;
    if (!p || (p->map_dtype != VP8HIP_SSIM_F16 && p->map_dtype != VP8HIP_SSIM_F32) || !ssim_planes(c, p->planes, L, elems)) return 0;
    return elems * (p->map_dtype == VP8HIP_SSIM_F32 ? 4 : 2);
}

extern "C" int vp8hip_ssim_share(const vp8hip_ctx *c, int n, unsigned planes)
{
    SsimLaunch L;
    size_t elems = 0;
    return n >= 1 && ssim_planes(c, planes, L, elems) ? ssim_share(n, L.pieces) : 0;
}

extern "C" int vp8hip_frames_ssim_async(vp8hip_ctx *c, const vp8hip_hist_job *jobs, int n, const vp8hip_ssim *p, void *scores, size_t scores_stride,
                                        void *map, size_t map_stride)
{
    const char *who = "vp8hip_frames_ssim_async";
    if (!c || !jobs || n < 1 || !p || (!scores && !map) || !c->width || c->fb.empty()) return fail(c, -2, "%s: bad arguments", who);
    if (int rc = vp8hip_check_pairs(c, who, jobs, n, false)) return rc;
    SsimLaunch L;
    memset(&L, 0, sizeof(L) - sizeof(L.j));
    size_t map_elems = 0;
    if (!ssim_planes(c, p->planes, L, map_elems)) return fail(c, -2, "%s: planes 0x%x (at least one of 0x%x)", who, p->planes, VP8HIP_HIST_YUV);
    const int dt = p->map_dtype;
    if (dt != VP8HIP_SSIM_F16 && dt != VP8HIP_SSIM_F32 && (dt != 0 || map)) return fail(c, -2, "%s: map_dtype %d", who, dt);
    if (map && !map_elems) return fail(c, -2, "%s: a map of planes without windows", who);
    const size_t es = dt == VP8HIP_SSIM_F32 ? 4 : 2, map_size = map_elems * es, scores_size = vp8hip_ssim_scores_size(L.np);
    if (scores)
        if (int rc = vp8hip_check_named_dst(c, who, "scores", scores, scores_stride, scores_size, 8, n)) return rc;
    if (map)
        if (int rc = vp8hip_check_named_dst(c, who, "map", map, map_stride, map_size, es, n)) return rc;
    if (scores && map && vp8hip_spans_overlap(scores, scores_stride, n, map, map_stride, n)) return fail(c, -2, "%s: scores and map overlap", who);
    HIPCHK(c, hipSetDevice(c->device));

    vp8hip_frame_planes(c, L);
    L.S = ssim_share(n, L.pieces);
    L.scores = scores != nullptr;
    L.map_dtype = map ? dt : 0;
    SsimFill F;
    F.np = L.np;
    for (int k = 0; k < 3; k++) F.count[k] = k < L.np ? (long long)L.p[k].nwx * L.p[k].nwy : 0;
    for (int i0 = 0; i0 < n; i0 += SSIM_MAX_JOBS) {
        const int m = n - i0 < SSIM_MAX_JOBS ? n - i0 : SSIM_MAX_JOBS;
        for (int k = 0; k < m; k++) {
            L.j[k].fb = vp8hip_frame_ref(c, jobs[i0 + k].fb);
            L.j[k].ref = vp8hip_frame_ref(c, jobs[i0 + k].ref_fb);
        }
        uint8_t *ds = scores ? (uint8_t *)scores + scores_stride * (size_t)i0 : nullptr;
        uint8_t *dm = map ? (uint8_t *)map + map_stride * (size_t)i0 : nullptr;
        if (scores && L.S > 1) {
            hipLaunchKernelGGL(vp8_ssim_fill_kernel, dim3(1, (unsigned)m), dim3(64), 0, c->stream, ds, scores_stride, F);
            HIPCHK(c, hipGetLastError());
        }
        hipLaunchKernelGGL(vp8_ssim_frames_kernel, dim3((unsigned)L.S, (unsigned)m), dim3(256), 0, c->stream, (const uint8_t *)c->fb_block,
                           c->fb_stride, (const uint8_t *)c->tile_block, c->tile_frame, ds, scores_stride, dm, map_stride, L);
        HIPCHK(c, hipGetLastError());
    }
    return 0;
}
