// What the calls that hand something to a device consumer share on the host (vp8hip_frames_scale_async, _rgb_async, _side_async,
// _residual_async, _coef_async, of vp8hip_trace.hip vp8hip_frames_trace_async, vp8hip_trace_flow_async, _residual_async,
// _gather_async, vp8hip_frames_wear_async, vp8hip_trace_wear_async, and the three that read picture pairs, vp8hip_frames_hist_async,
// _ssim_async and _motion_async): the checks of their lists, of picture pairs, of the output grid and of a destination in the
// caller's device memory, named where a call has several; where the planes of the frame buffers lie; and what a kernel needs of a
// slot's quantiser header.  Every check returns 0, or -2 with the error set, its text begun with `who`, the calling function's
// name; none enqueues anything.
#include "vp8hip_ctx.hip.h"

// n frame buffers of the context
int vp8hip_check_fbs(vp8hip_ctx *c, const char *who, const int *fbs, int n)
{
    for (int i = 0; i < n; i++)
        if (fbs[i] < 0 || fbs[i] >= (int)c->fb.size()) return fail(c, -2, "%s: frame buffer %d out of range", who, fbs[i]);
    return 0;
}

// n picture pairs of the context, job by job fb, then ref_fb; ref_optional: a ref_fb of exactly -1 names none
int vp8hip_check_pairs(vp8hip_ctx *c, const char *who, const vp8hip_hist_job *jobs, int n, bool ref_optional)
{
    for (int i = 0; i < n; i++) {
        if (int rc = vp8hip_check_fbs(c, who, &jobs[i].fb, 1)) return rc;
        if (ref_optional && jobs[i].ref_fb == -1) continue;
        if (int rc = vp8hip_check_fbs(c, who, &jobs[i].ref_fb, 1)) return rc;
    }
    return 0;
}

// where the planes of the context's frame buffers lie, for the kernels that read them in either form (vp8_frame_read.hip.h)
void vp8hip_frame_planes(const vp8hip_ctx *c, FramePlanes &L)
{
    L.dw = c->width; L.dh = c->height;
    L.mb_cols = c->dg.mb_cols; L.mb_rows = c->dg.mb_rows;
    L.y_off = c->dg.y_off; L.u_off = c->dg.u_off; L.v_off = c->dg.v_off;
    L.y_stride = c->dg.y_stride; L.uv_stride = c->dg.uv_stride;
}

// n IR slots of the context, each holding a frame of the context's size (as of its last upload / copy / entropy launch)
int vp8hip_check_slots(vp8hip_ctx *c, const char *who, const int *slots, int n)
{
    for (int i = 0; i < n; i++) {
        if (slots[i] < 0 || slots[i] >= (int)c->slots.size()) return fail(c, -2, "%s: slot %d out of range", who, slots[i]);
        const vp8ir_frame_hdr &h = c->slots[slots[i]].hdr_copy;
        if (h.mb_cols != c->dg.mb_cols || h.mb_rows != c->dg.mb_rows)
            return fail(c, -2, "%s: slot %d holds no frame of the context's size", who, slots[i]);
    }
    return 0;
}

// The output grid of dst_w x dst_h: both 0 for the native grid of context c (null, or not configured: refused), `cells` a macroblock
// each way (4: luma blocks, 16: samples); otherwise 1..VP8HIP_MAX_OUT_SIZE each.  False for what is refused.
bool vp8hip_out_grid(const vp8hip_ctx *c, int dst_w, int dst_h, int cells, int &gw, int &gh)
{
    if (dst_w == 0 && dst_h == 0) {
        if (!c || !c->width) return false;
        gw = cells * c->dg.mb_cols; gh = cells * c->dg.mb_rows;
        return true;
    }
    if (dst_w < 1 || dst_h < 1 || dst_w > VP8HIP_MAX_OUT_SIZE || dst_h > VP8HIP_MAX_OUT_SIZE) return false;
    gw = dst_w; gh = dst_h;
    return true;
}

// the destination of n frames of `size` bytes, dst_stride apart: device memory of this context's device, inside one allocation
int vp8hip_check_device_span(vp8hip_ctx *c, const char *who, const void *dst, size_t dst_stride, size_t size, int n)
{
    HIPCHK(c, hipSetDevice(c->device));
    hipPointerAttribute_t pa;
    memset(&pa, 0, sizeof pa);
    if (hipPointerGetAttributes(&pa, dst) != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, -2, "%s: the destination is not memory HIP knows", who);
    }
    if (pa.type != hipMemoryTypeDevice || pa.device != c->device)
        return fail(c, -2, "%s: the destination is not device memory of device %d", who, c->device);
    hipDeviceptr_t abase = nullptr;
    size_t asize = 0;
    if (hipMemGetAddressRange(&abase, &asize, (hipDeviceptr_t)dst) != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, -2, "%s: no allocation holds the destination", who);
    }
    const uintptr_t a0 = (uintptr_t)abase, d0 = (uintptr_t)dst;
    const bool wraps = dst_stride > (SIZE_MAX - size) / (size_t)n;
    const size_t span = wraps ? SIZE_MAX : dst_stride * (size_t)(n - 1) + size;
    if (wraps || d0 < a0 || (d0 - a0) > asize || span > asize - (d0 - a0))
        return fail(c, -2, "%s: %d frames of %zu bytes, %zu apart, do not fit in the destination's allocation", who, n, size,
                    dst_stride);
    return 0;
}

// ... and, before that: a stride of at least the frame; destination and stride aligned to the element of elem_size bytes
int vp8hip_check_dst(vp8hip_ctx *c, const char *who, const void *dst, size_t dst_stride, size_t size, size_t elem_size, int n)
{
    if (dst_stride < size) return fail(c, -2, "%s: stride %zu below the frame's %zu bytes", who, dst_stride, size);
    if ((uintptr_t)dst % elem_size || dst_stride % elem_size)
        return fail(c, -2, "%s: destination %p / stride %zu not aligned to the %zu-byte element", who, dst, dst_stride, elem_size);
    return vp8hip_check_device_span(c, who, dst, dst_stride, size, n);
}

// ... of a call that has several destinations: the texts begin with "`who` (`name`)"
int vp8hip_check_named_dst(vp8hip_ctx *c, const char *who, const char *name, const void *dst, size_t dst_stride, size_t size, size_t elem_size, int n)
{
    char who_dst[64];
    snprintf(who_dst, sizeof(who_dst), "%s (%s)", who, name);
    return vp8hip_check_dst(c, who_dst, dst, dst_stride, size, elem_size, n);
}

// the quantiser index of each segment (mb_init_dequantizer, vp8/decoder/decodframe.c), segment s in bits 7s .. 7s + 6
unsigned vp8hip_segment_q_bits(const vp8ir_frame_hdr &h)
{
    unsigned q = 0;
    for (int s = 0; s < 4; s++) {
        int qi = h.base_qindex;
        if (h.segmentation_enabled) qi = h.mb_segment_abs_delta ? h.segment_quant[s] : qi + h.segment_quant[s];
        qi = qi < 0 ? 0 : qi > 127 ? 127 : qi;
        q |= (unsigned)qi << (7 * s);
    }
    return q;
}
