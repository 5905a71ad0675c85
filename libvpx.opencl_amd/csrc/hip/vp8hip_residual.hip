// vp8hip_frames_residual_async (include/vp8hip.h): the decoded residual of IR slots as tensors in the caller's device memory.  The
// plan is made here, once per call; the kernels are in vp8_residual.hip.  Everything they read is in the slots (records and block
// stream; on a vp8hip_configure_pooled context the blocks lie in the pool) or comes with the launch (the slots' quantiser header
// as of this call): nothing is allocated, copied or synchronised.
#include "vp8hip_ctx.hip.h"

#define RES_ARGS const char *slot_base, size_t slot_bytes, size_t o_mbx, size_t o_blocks, const char *pool, unsigned cap_blocks, uint8_t *dst, \
                 size_t dst_stride, ResLaunch L
extern "C" __global__ void vp8_residual_i16_kernel(RES_ARGS);
extern "C" __global__ void vp8_residual_f16_kernel(RES_ARGS);
extern "C" __global__ void vp8_residual_f32_kernel(RES_ARGS);

#define RES_PART_ROWS 64                        // output rows of a workgroup where a grid is much taller than the frame
static_assert(sizeof(ResLaunch) < 3072, "the kernel arguments stay well under 4 KB");

// the grid of p on context c (null: sized grids only); false for what the call refuses on p alone
static bool res_grid(const vp8hip_ctx *c, const vp8hip_residual *p, int &gw, int &gh, int &cw, int &ch)
{
    if (!p || p->dtype < 0 || p->dtype > 2 || (p->layout != VP8HIP_RES_I420 && p->layout != VP8HIP_RES_PLANAR)) return false;
    if (!vp8hip_out_grid(c, p->dst_w, p->dst_h, 16, gw, gh)) return false;
    cw = (gw + 1) / 2; ch = (gh + 1) / 2;        // (the native grid is even both ways)
    return true;
}

static size_t res_size(const vp8hip_residual *p, int gw, int gh, int cw, int ch)
{
    const size_t elems = p->layout == VP8HIP_RES_PLANAR ? (size_t)3 * gh * gw : (size_t)gh * gw + (size_t)2 * ch * cw;
    return elems * vp8hip_elem_size(p->dtype, 2);
}

extern "C" size_t vp8hip_residual_size(const vp8hip_ctx *c, const vp8hip_residual *p)
{
    int gw, gh, cw, ch;
    return res_grid(c, p, gw, gh, cw, ch) ? res_size(p, gw, gh, cw, ch) : 0;
}

// what the kernel needs of a slot's header: the quantiser index of each segment, and the five *_delta_q as the header holds them
// (bytes: a header built by hand may hold any int8)
ResSlot vp8hip_res_header_bits(int slot, const vp8ir_frame_hdr &h)
{
    ResSlot s;
    s.slot = slot;
    s.q = vp8hip_segment_q_bits(h);
    s.d0 = (unsigned)(uint8_t)h.y1dc_delta_q | (unsigned)(uint8_t)h.y2dc_delta_q << 8 | (unsigned)(uint8_t)h.y2ac_delta_q << 16 |
           (unsigned)(uint8_t)h.uvdc_delta_q << 24;
    s.d1 = (unsigned)(uint8_t)h.uvac_delta_q;
    return s;
}

// The launch for a grid of gw x gh: the sizes the luma and chroma grids are laid over, the runs of a macroblock row and how many
// workgroups share a run's output rows.
static void residual_plan(const vp8hip_ctx *c, const vp8hip_residual &p, int gw, int gh, int cw, int ch, ResLaunch &L)
{
    const bool native = p.dst_w == 0;
    memset(&L, 0, offsetof(ResLaunch, s));
    L.gw = gw; L.gh = gh; L.cw = cw; L.ch = ch;
    L.dw = native ? 16 * c->dg.mb_cols : c->width;
    L.dh = native ? 16 * c->dg.mb_rows : c->height;
    L.dcw = (L.dw + 1) / 2; L.dch = (L.dh + 1) / 2;
    L.mb_cols = c->dg.mb_cols; L.mb_rows = c->dg.mb_rows;
    L.runs = (L.mb_cols + RES_RUN - 1) / RES_RUN;
    // output rows a macroblock row can have: 16 source rows, stretched
    const long long most = ((long long)16 * gh + L.dh - 1) / L.dh + 1;
    L.S = (int)((most + RES_PART_ROWS - 1) / RES_PART_ROWS);
    if (L.S > gh) L.S = gh;
    L.layout = p.layout;
    for (int k = 0; k < 3; k++) L.scale[k] = p.scale[k];
}

extern "C" int vp8hip_frames_residual_async(vp8hip_ctx *c, const int *slots, int n, const vp8hip_residual *p, void *dst, size_t dst_stride)
{
    const char *who = "vp8hip_frames_residual_async";
    if (!c || !slots || n < 1 || !p || !dst || c->slots.empty()) return fail(c, -2, "%s: bad arguments", who);
    if (int rc = vp8hip_check_slots(c, who, slots, n)) return rc;
    int gw, gh, cw, ch;
    if (!res_grid(c, p, gw, gh, cw, ch))
        return fail(c, -2, "%s: grid %dx%d (both 0, or 1..%d each), layout %d, type %d", who, p->dst_w, p->dst_h, VP8HIP_MAX_OUT_SIZE, p->layout,
                    p->dtype);
    const size_t es = (size_t)vp8hip_elem_size(p->dtype, 2), size = res_size(p, gw, gh, cw, ch);
    if (int rc = vp8hip_check_dst(c, who, dst, dst_stride, size, es, n)) return rc;
    HIPCHK(c, hipSetDevice(c->device));

    ResLaunch L;
    residual_plan(c, *p, gw, gh, cw, ch, L);
    void (*const kernels[3])(RES_ARGS) = {vp8_residual_i16_kernel, vp8_residual_f16_kernel, vp8_residual_f32_kernel};
    void (*const kernel)(RES_ARGS) = kernels[p->dtype];
    const size_t piece = 4 * es;
    const bool aligned = (uintptr_t)dst % piece == 0 && dst_stride % piece == 0;
    L.y_vec = aligned && gw % 4 == 0;
    // (the chroma planes of the I420 layout begin behind gh * gw elements: aligned to the piece when gw % 4 == 0, or by chance)
    L.c_vec = aligned && cw % 4 == 0 && ((size_t)gh * gw * es) % piece == 0;
    const size_t cap = c->pool ? ((size_t)c->pool_chunks + 1) * c->chunk_blocks : c->cap_blocks;
    // (the kernel clamps a block's index to cap - 1, as 32 bits: what keeps a starved slot's reads in bounds)
    if (cap < 1 || cap > 0xffffffffull) return fail(c, -2, "%s: a block stream of %zu blocks", who, cap);
    const unsigned groups = (unsigned)(L.mb_rows * L.runs * L.S);
    for (int i0 = 0; i0 < n; i0 += RES_MAX_FRAMES) {
        const int m = n - i0 < RES_MAX_FRAMES ? n - i0 : RES_MAX_FRAMES;
        for (int k = 0; k < m; k++) L.s[k] = vp8hip_res_header_bits(slots[i0 + k], c->slots[slots[i0 + k]].hdr_copy);
        hipLaunchKernelGGL(kernel, dim3(groups, (unsigned)m), dim3(256), 0, c->stream, (const char *)c->slot_block_dev, c->slot_bytes, c->o_mbx,
                           c->o_blocks, (const char *)c->pool, (unsigned)cap, (uint8_t *)dst + dst_stride * (size_t)i0, dst_stride, L);
        HIPCHK(c, hipGetLastError());
    }
    return 0;
}
