// vp8hip_frames_rgb_async (include/vp8hip.h): decoded frames as RGB tensors in the caller's device memory.  The plan is made here,
// once per call; the kernels are in vp8_rgb.hip.  At the display size they read the frames; at any other size the scaler
// (vp8hip_scale.hip) first writes a chunk of frames as packed I420 into a scratch the context keeps, and they read that.
#include "vp8hip_ctx.hip.h"

#define RGB_ARGS const uint8_t *raster, size_t fb_stride, const uint8_t *tiles, size_t tile_frame, const uint8_t *packed, size_t packed_stride, \
                 uint8_t *dst, size_t dst_stride, RgbLaunch L
extern "C" __global__ void vp8_rgb_planar_u8_kernel(RGB_ARGS);
extern "C" __global__ void vp8_rgb_planar_f16_kernel(RGB_ARGS);
extern "C" __global__ void vp8_rgb_planar_f32_kernel(RGB_ARGS);
extern "C" __global__ void vp8_rgb_packed3_u8_kernel(RGB_ARGS);
extern "C" __global__ void vp8_rgb_packed3_f16_kernel(RGB_ARGS);
extern "C" __global__ void vp8_rgb_packed3_f32_kernel(RGB_ARGS);
extern "C" __global__ void vp8_rgb_packed4_u8_kernel(RGB_ARGS);

#define RGB_SCRATCH_MAX ((size_t)256 << 20)     // the scratch holds one chunk of frames: at most this much (one frame at least)
#define RGB_BAND_LDS 24576                      // rows of a band in LDS: six workgroups to a CU beside the value table

// yoff, cy, crv, cgu, cgv, cbu: the exact matrices times 256, rounded
static const int rgb_matrix[3][6] = {
    {16, 298, 409, -100, -208, 516},            // BT.601, limited range
    {0, 256, 359, -88, -183, 454},              // BT.601, full range
    {16, 298, 459, -55, -136, 541},             // BT.709, limited range
};

// the kernels' coefficients of a matrix (VP8HIP_RGB_BT601 ...: 0..2), by POSITION (order 1 swaps the first and the third channel):
// the byte at position p = clamp255((cy * Y + k0 + cu[p] * (U - 128) + cv[p] * (V - 128)) >> 8)
void vp8hip_rgb_coeffs(int matrix, int order, int &cy, int &k0, int (&cu)[3], int (&cv)[3])
{
    const int *m = rgb_matrix[matrix];
    cy = m[1];
    k0 = 128 - m[1] * m[0];
    const int ucol[3] = {0, m[3], m[5]}, vcol[3] = {m[2], m[4], 0};
    for (int pos = 0; pos < 3; pos++) {
        const int col = order ? 2 - pos : pos;
        cu[pos] = ucol[col]; cv[pos] = vcol[col];
    }
}

extern "C" size_t vp8hip_rgb_size(const vp8hip_rgb *p)
{
    if (!p || p->dst_w < 1 || p->dst_h < 1 || p->dst_w > VP8HIP_MAX_OUT_SIZE || p->dst_h > VP8HIP_MAX_OUT_SIZE) return 0;
    if (p->filter < 0 || p->filter > 2 || p->matrix < 0 || p->matrix > 2 || p->layout < 0 || p->layout > 2 || p->order < 0 || p->order > 1 ||
        p->dtype < 0 || p->dtype > 2)
        return 0;
    if (p->layout == VP8HIP_RGB_PACKED4 && p->dtype != VP8HIP_RGB_U8) return 0;
    return (size_t)p->dst_w * p->dst_h * (p->layout == VP8HIP_RGB_PACKED4 ? 4 : 3) * vp8hip_elem_size(p->dtype, 1);
}

extern "C" size_t vp8hip_rgb_scratch_bytes(const vp8hip_ctx *c) { return c ? c->d_rgb.cap : 0; }

// bytes between two images of the scratch: a multiple of 16, with room for the dword a row's last load may run into
static size_t rgb_image_stride(int w, int h) { return align_up(vp8hip_i420_size(w, h) + 4, 16); }

// The launch for images of sw x sh: the source planes as they lie in a frame buffer (the display size) or in a packed image, the
// band height, the coefficients and the table's arguments by POSITION (order 1 swaps the first and the third channel).  Returns the
// LDS a workgroup takes.
static int rgb_plan(const vp8hip_ctx *c, const vp8hip_rgb &p, bool from_frames, uintptr_t dst, size_t dst_stride, RgbLaunch &L)
{
    const int w = p.dst_w, h = p.dst_h;
    memset(&L, 0, offsetof(RgbLaunch, fb));
    if (from_frames) {
        ScaleLaunch S;
        (void)vp8hip_scale_plan(c, w, h, 0, S);           // (the copy's planes: origin, stride, aligned area and slot width of each)
        for (int pl = 0; pl < 3; pl++) L.p[pl] = S.p[pl];
    } else {
        const int cw = (w + 1) >> 1, ch = (h + 1) >> 1;
        for (int pl = 0; pl < 3; pl++) {
            ScalePlane &P = L.p[pl];
            P.aw = P.sw = P.dw = pl ? cw : w;
            P.ah = P.sh = P.dh = pl ? ch : h;
            P.src_off = pl == 0 ? 0 : w * h + (pl - 1) * cw * ch;
            P.src_stride = P.aw;
            P.tile_plane = pl;
            P.rw = (P.aw + 16 + 15) & ~15;
        }
    }
    L.w = w; L.h = h;
    L.mb_cols = c->dg.mb_cols;
    const int per2 = 2 * L.p[0].rw + 2 * L.p[1].rw;       // two luma rows and a row of each chroma plane
    int pairs = RGB_BAND_LDS / per2;
    pairs = pairs < 1 ? 1 : pairs > 32 ? 32 : pairs;      // (two rows of the widest frame: 49 KB)
    if (pairs > (h + 1) / 2) pairs = (h + 1) / 2;
    L.br = 2 * pairs;
    vp8hip_rgb_coeffs(p.matrix, p.order, L.cy, L.k0, L.cu, L.cv);
    for (int pos = 0; pos < 3; pos++) {
        const int col = p.order ? 2 - pos : pos;
        L.scale[pos] = p.scale[col]; L.bias[pos] = p.bias[col];
    }
    const int es = vp8hip_elem_size(p.dtype, 1);
    const size_t piece = p.layout == VP8HIP_RGB_PACKED4 ? 16 : (size_t)4 * es;
    L.vec = w % 4 == 0 && dst % piece == 0 && dst_stride % piece == 0;
    return (p.dtype == VP8HIP_RGB_U8 ? 0 : 3072) + pairs * per2;
}

extern "C" int vp8hip_frames_rgb_async(vp8hip_ctx *c, const int *fbs, int n, const vp8hip_rgb *p, void *dst, size_t dst_stride)
{
    const char *who = "vp8hip_frames_rgb_async";
    if (!c || !fbs || n < 1 || !p || !dst || c->fb.empty()) return fail(c, -2, "%s: bad arguments", who);
    if (int rc = vp8hip_check_fbs(c, who, fbs, n)) return rc;
    if (p->dst_w < 1 || p->dst_h < 1 || p->dst_w > VP8HIP_MAX_OUT_SIZE || p->dst_h > VP8HIP_MAX_OUT_SIZE)
        return fail(c, -2, "%s: size %dx%d outside 1..%d", who, p->dst_w, p->dst_h, VP8HIP_MAX_OUT_SIZE);
    const size_t size = vp8hip_rgb_size(p);
    if (!size)
        return fail(c, -2, "%s: filter %d, matrix %d, layout %d, order %d, dtype %d (four-byte pixels: bytes only)", who, p->filter, p->matrix,
                    p->layout, p->order, p->dtype);
    if (int rc = vp8hip_check_dst(c, who, dst, dst_stride, size, (size_t)vp8hip_elem_size(p->dtype, 1), n)) return rc;

    const bool from_frames = p->dst_w == c->width && p->dst_h == c->height;
    // the chunk: what the kernel arguments carry, and -- scaled -- what the scratch holds
    int chunk = n < SCALE_MAX_FRAMES ? n : SCALE_MAX_FRAMES;
    size_t istride = 0;
    ScaleLaunch S;
    int scale_lds = 0;
    if (!from_frames) {
        istride = rgb_image_stride(p->dst_w, p->dst_h);
        const size_t fit = RGB_SCRATCH_MAX / istride;
        if ((size_t)chunk > fit) chunk = fit < 1 ? 1 : (int)fit;
        const size_t need = istride * (size_t)chunk;
        // (launches in flight read the scratch: hipFree waits for them)
        if (c->d_rgb.grow(need) != hipSuccess)
            return fail(c, -1, "vp8hip_frames_rgb_async: no device memory for %zu bytes of scratch", need);
        scale_lds = vp8hip_scale_plan(c, p->dst_w, p->dst_h, p->filter, S);
    }
    RgbLaunch L;
    const int lds = rgb_plan(c, *p, from_frames, (uintptr_t)dst, dst_stride, L);
    void (*const kernels[3][3])(RGB_ARGS) = {
        {vp8_rgb_planar_u8_kernel, vp8_rgb_planar_f16_kernel, vp8_rgb_planar_f32_kernel},
        {vp8_rgb_packed3_u8_kernel, vp8_rgb_packed3_f16_kernel, vp8_rgb_packed3_f32_kernel},
        {vp8_rgb_packed4_u8_kernel, nullptr, nullptr},
    };
    void (*const kernel)(RGB_ARGS) = kernels[p->layout][p->dtype];
    const unsigned bands = (unsigned)((p->dst_h + L.br - 1) / L.br);
    for (int i0 = 0; i0 < n; i0 += chunk) {
        const int m = n - i0 < chunk ? n - i0 : chunk;
        if (from_frames) {
            for (int k = 0; k < m; k++) L.fb[k] = vp8hip_frame_ref(c, fbs[i0 + k]);
        } else {
            if (int rc = vp8hip_scale_enqueue(c, fbs + i0, m, S, scale_lds, c->d_rgb, istride)) return rc;
            for (int k = 0; k < m; k++) L.fb[k] = SCALE_FROM_PACKED;
        }
        hipLaunchKernelGGL(kernel, dim3(bands, (unsigned)m), dim3(256), (unsigned)lds, c->stream, (const uint8_t *)c->fb_block, c->fb_stride,
                           (const uint8_t *)c->tile_block, c->tile_frame, (const uint8_t *)c->d_rgb, istride,
                           (uint8_t *)dst + dst_stride * (size_t)i0, dst_stride, L);
        HIPCHK(c, hipGetLastError());
    }
    return 0;
}
