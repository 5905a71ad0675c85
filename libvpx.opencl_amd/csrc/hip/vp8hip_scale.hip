// vp8hip_frames_scale_async (include/vp8hip.h): decoded frames as packed I420 in the caller's device memory, at the display size or
// scaled as libyuv's I420Scale scales them (third_party/libyuv/source/scale.c:3762).  The plan is made here, once per call; the
// kernel is in vp8_scale.hip.
#include "vp8hip_ctx.hip.h"

extern "C" __global__ void vp8_scale_kernel(const uint8_t *raster, size_t fb_stride, const uint8_t *tiles, size_t tile_frame, uint8_t *dst,
                                            size_t dst_stride, ScaleLaunch L);

extern "C" size_t vp8hip_i420_size(int w, int h)
{
    if (w < 1 || h < 1 || w > VP8HIP_MAX_OUT_SIZE || h > VP8HIP_MAX_OUT_SIZE) return 0;
    return (size_t)w * h + 2 * (size_t)((w + 1) / 2) * ((h + 1) / 2);
}

extern "C" int vp8hip_device(const vp8hip_ctx *c) { return c ? c->device : -1; }

// The whole dispatch of I420Scale for one frame geometry (returns the LDS a workgroup needs): ScalePlane (scale.c:3702) per plane -- chroma on its own sizes,
// (v + 1) >> 1 on both sides -- with the parameters of the path it takes.  kFilterBox goes where kFilterBilinear goes:
// ScalePlaneDown tests src_height * 2 > dst_height (scale.c:3664), true for every downscale.
int vp8hip_scale_plan(const vp8hip_ctx *c, int dw, int dh, int filter, ScaleLaunch &L)
{
    const int w = c->width, h = c->height;
    const vp8ir_geom &g = c->geom;
    int doff = 0, blk = 0, lds = 0;
    for (int pl = 0; pl < 3; pl++) {
        ScalePlane &P = L.p[pl];
        memset(&P, 0, sizeof P);
        const int sw = pl ? (w + 1) >> 1 : w, sh = pl ? (h + 1) >> 1 : h;
        const int tw = pl ? (dw + 1) >> 1 : dw, th = pl ? (dh + 1) >> 1 : dh;
        const bool f = filter != 0;
        P.sw = sw; P.sh = sh; P.dw = tw; P.dh = th;
        P.aw = pl ? g.aligned_w / 2 : g.aligned_w;
        P.ah = pl ? g.aligned_h / 2 : g.aligned_h;
        P.src_off = pl == 0 ? g.y_off : pl == 1 ? g.u_off : g.v_off;
        P.src_stride = pl ? g.uv_stride : g.y_stride;
        P.tile_plane = pl;
        P.filt = 0;
        if (tw == sw && th == sh) P.path = SCALE_COPY;
        else if (tw <= sw && th <= sh && 4 * tw == 3 * sw && 4 * th == 3 * sh) { P.path = SCALE_DOWN34; P.filt = f; }
        else if (tw <= sw && th <= sh && 2 * tw == sw && 2 * th == sh) { P.path = SCALE_DOWN2; P.filt = f; }
        else if (tw <= sw && th <= sh && 8 * tw == 3 * sw && th == (sh * 3 + 7) / 8) { P.path = SCALE_DOWN38; P.filt = f; }
        else if (tw <= sw && th <= sh && 4 * tw == sw && 4 * th == sh) { P.path = SCALE_DOWN4; P.filt = f; }
        else if (tw <= sw && th <= sh && 8 * tw == sw && 8 * th == sh) { P.path = SCALE_DOWN8; P.filt = f && tw <= 640; }  // kMaxOutputWidth
        else if (!f) P.path = SCALE_POINT;                                      // ScalePlaneSimple
        else if (sw % 8 == 0 && sw <= 2560) { P.path = SCALE_BILIN8; P.filt = 1; }    // kMaxInputWidth (scale.c:3553)
        else { P.path = SCALE_BILIN16; P.filt = 1; }                           // ScalePlaneBilinearSimple
        P.dx = (sw << 16) / tw;
        P.dy = (sh << 16) / th;
        P.maxx = ((sw - 1) << 16) - 1;
        P.maxy = ((sh - 1) << 16) - 1;
        P.x0 = tw < sw ? 32768 : (sw << 16) / tw - 32768;
        P.y0 = th < sh ? 32768 : (sh << 16) / th - 32768;
        P.doff = doff;
        P.dsize = tw * th;
        P.adv_rows = SCALE_WIN * 256 / tw;
        P.adv_cols = SCALE_WIN * 256 - P.adv_rows * tw;
        P.blk0 = blk;
        doff += P.dsize;
        // a workgroup per band of br output rows whose source rows -- nr per output row -- fit in 32 KB of LDS (64 KB where one row's
        // do not); planes wider than that: a workgroup per 256 dwords of the destination that meet the plane (at most dsize / 4 + 2)
        P.nr = P.path == SCALE_BILIN8 || P.path == SCALE_BILIN16 ? 2
             : !P.filt ? 1 : P.path == SCALE_DOWN2 || P.path == SCALE_DOWN34 ? 2 : P.path == SCALE_DOWN4 ? 4 : P.path == SCALE_DOWN8 ? 8
             : P.path == SCALE_DOWN38 ? 3 : 1;
        P.rw = (P.aw + 16 + 15) & ~15;
        const int per_row = P.nr * P.rw;
        int br = (SCALE_MAX_LDS / 2) / per_row;
        if (br < 1) br = SCALE_MAX_LDS / per_row;
        P.br = br < 1 ? 0 : br > 64 ? 64 : br > th ? th : br;
        blk += P.br ? (th + P.br - 1) / P.br : (P.dsize / SCALE_WIN + 2 + 255) / 256;
        if (P.br && P.br * per_row > lds) lds = P.br * per_row;
    }
    L.blocks = blk;
    L.mb_cols = c->dg.mb_cols;
    return lds;
}

// m <= SCALE_MAX_FRAMES frames of a planned call on the context's stream; each frame is read in a form it has: raster where it
// exists, else tiles; never converted
int vp8hip_scale_enqueue(vp8hip_ctx *c, const int *fbs, int m, ScaleLaunch &L, int lds, void *dst, size_t dst_stride)
{
    for (int k = 0; k < m; k++) L.fb[k] = vp8hip_frame_ref(c, fbs[k]);
    hipLaunchKernelGGL(vp8_scale_kernel, dim3((unsigned)L.blocks, (unsigned)m), dim3(256), (unsigned)lds, c->stream, (const uint8_t *)c->fb_block,
                       c->fb_stride, (const uint8_t *)c->tile_block, c->tile_frame, (uint8_t *)dst, dst_stride, L);
    HIPCHK(c, hipGetLastError());
    return 0;
}

extern "C" int vp8hip_frames_scale_async(vp8hip_ctx *c, const int *fbs, int n, int dst_w, int dst_h, int filter, void *dst, size_t dst_stride)
{
    const char *who = "vp8hip_frames_scale_async";
    if (!c || !fbs || n < 1 || !dst || c->fb.empty()) return fail(c, -2, "%s: bad arguments", who);
    if (int rc = vp8hip_check_fbs(c, who, fbs, n)) return rc;
    const size_t size = vp8hip_i420_size(dst_w, dst_h);
    if (!size) return fail(c, -2, "%s: size %dx%d outside 1..%d", who, dst_w, dst_h, VP8HIP_MAX_OUT_SIZE);
    if (filter < 0 || filter > 2) return fail(c, -2, "%s: filter %d (0 none, 1 bilinear, 2 box)", who, filter);
    if (int rc = vp8hip_check_dst(c, who, dst, dst_stride, size, 1, n)) return rc;

    ScaleLaunch L;
    const int lds = vp8hip_scale_plan(c, dst_w, dst_h, filter, L);       // (bytes of LDS a workgroup takes)
    for (int i0 = 0; i0 < n; i0 += SCALE_MAX_FRAMES) {
        const int m = n - i0 < SCALE_MAX_FRAMES ? n - i0 : SCALE_MAX_FRAMES;
        if (int rc = vp8hip_scale_enqueue(c, fbs + i0, m, L, lds, (uint8_t *)dst + dst_stride * (size_t)i0, dst_stride)) return rc;
    }
    return 0;
}
