// vp8hip_frames_side_async (include/vp8hip.h): motion vectors and macroblock modes of IR slots as tensors in the caller's device
// memory.  The plan is made here, once per call; the kernels are in vp8_side.hip.  Everything they read is in the slots (records
// and vectors: also on a vp8hip_configure_pooled context) or comes with the launch (the slots' header bits as of this call):
// nothing is allocated, copied or synchronised.
#include "vp8hip_ctx.hip.h"

#define SIDE_ARGS const char *slot_base, size_t slot_bytes, size_t o_mbx, size_t o_mvs, uint8_t *mv_dst, size_t mv_stride, uint8_t *info_dst, \
                  size_t info_stride, SideLaunch L
extern "C" __global__ void vp8_side_i16_kernel(SIDE_ARGS);
extern "C" __global__ void vp8_side_f16_kernel(SIDE_ARGS);
extern "C" __global__ void vp8_side_f32_kernel(SIDE_ARGS);

#define SIDE_ALL_PLANES 63u
#define SIDE_GROUP_LDS 32768                    // records and vectors of a group of macroblock rows: five workgroups to a CU ...
#define SIDE_GROUP_ROWS 4                       // ... and at most this many rows (small frames: more workgroups)
#define SIDE_PART_ROWS 64                       // output rows of a workgroup where a grid is much taller than the frame

static int side_nplanes(unsigned planes) { return __builtin_popcount(planes); }

// the grid of p on context c (null: sized grids only); false for what the call refuses on p alone
static bool side_grid(const vp8hip_ctx *c, const vp8hip_side *p, int &gw, int &gh)
{
    if (!p || p->mv_dtype < 0 || p->mv_dtype > 2 || (p->planes & ~SIDE_ALL_PLANES)) return false;
    return vp8hip_out_grid(c, p->dst_w, p->dst_h, 4, gw, gh);
}

extern "C" size_t vp8hip_side_mv_size(const vp8hip_ctx *c, const vp8hip_side *p)
{
    int gw, gh;
    return side_grid(c, p, gw, gh) ? (size_t)2 * gh * gw * vp8hip_elem_size(p->mv_dtype, 2) : 0;
}

extern "C" size_t vp8hip_side_info_size(const vp8hip_ctx *c, const vp8hip_side *p)
{
    int gw, gh;
    return side_grid(c, p, gw, gh) ? (size_t)side_nplanes(p->planes) * gh * gw : 0;
}

// what the kernel needs of a slot's header: the quantiser index of each segment, and bit 28 for a key frame
unsigned vp8hip_side_header_bits(const vp8ir_frame_hdr &h) { return vp8hip_segment_q_bits(h) | (h.frame_type == 0 ? 1u << 28 : 0u); }

// The launch for a grid of gw x gh: the size it is laid over, the group of macroblock rows a workgroup stages and how many
// workgroups share a group's output rows.  Returns the LDS a workgroup takes.
static size_t side_plan(const vp8hip_ctx *c, const vp8hip_side &p, int gw, int gh, SideLaunch &L)
{
    const bool native = p.dst_w == 0;
    memset(&L, 0, offsetof(SideLaunch, slot));
    L.gw = gw; L.gh = gh;
    L.dw = native ? 16 * c->dg.mb_cols : c->width;
    L.dh = native ? 16 * c->dg.mb_rows : c->height;
    L.mb_cols = c->dg.mb_cols; L.mb_rows = c->dg.mb_rows;
    const size_t row_bytes = (size_t)L.mb_cols * 128;
    int R = (int)(SIDE_GROUP_LDS / row_bytes);
    R = R < 1 ? 1 : R > SIDE_GROUP_ROWS ? SIDE_GROUP_ROWS : R;
    if (R > L.mb_rows) R = L.mb_rows;
    L.R = R;
    // output rows a group can have: R * 16 source rows, stretched
    const long long most = ((long long)R * 16 * gh + L.dh - 1) / L.dh + 1;
    L.S = (int)((most + SIDE_PART_ROWS - 1) / SIDE_PART_ROWS);
    if (L.S > gh) L.S = gh;
    L.xmode = native ? SIDE_X_NATIVE : gw == c->width ? SIDE_X_DISPLAY : SIDE_X_ANY;
    L.planes = p.planes;
    L.scale[0] = p.scale[0]; L.scale[1] = p.scale[1];
    return (size_t)R * row_bytes;
}

extern "C" int vp8hip_frames_side_async(vp8hip_ctx *c, const int *slots, int n, const vp8hip_side *p, void *mv_dst, size_t mv_stride,
                                        void *info_dst, size_t info_stride)
{
    const char *who = "vp8hip_frames_side_async";
    if (!c || !slots || n < 1 || !p || (!mv_dst && !info_dst) || c->slots.empty()) return fail(c, -2, "%s: bad arguments", who);
    if (int rc = vp8hip_check_slots(c, who, slots, n)) return rc;
    int gw, gh;
    if (!side_grid(c, p, gw, gh))
        return fail(c, -2, "%s: grid %dx%d (both 0, or 1..%d each), type %d, planes 0x%x", who, p->dst_w, p->dst_h, VP8HIP_MAX_OUT_SIZE,
                    p->mv_dtype, p->planes);
    if (info_dst && !p->planes) return fail(c, -2, "%s: an info tensor of no planes", who);
    const size_t es = (size_t)vp8hip_elem_size(p->mv_dtype, 2);
    const size_t mv_size = (size_t)2 * gh * gw * es, info_size = (size_t)side_nplanes(p->planes) * gh * gw;
    if (mv_dst)
        if (int rc = vp8hip_check_dst(c, "vp8hip_frames_side_async (mv)", mv_dst, mv_stride, mv_size, es, n)) return rc;
    if (info_dst)
        if (int rc = vp8hip_check_dst(c, "vp8hip_frames_side_async (info)", info_dst, info_stride, info_size, 1, n)) return rc;
    HIPCHK(c, hipSetDevice(c->device));

    SideLaunch L;
    const size_t lds = side_plan(c, *p, gw, gh, L);
    void (*const kernels[3])(SIDE_ARGS) = {vp8_side_i16_kernel, vp8_side_f16_kernel, vp8_side_f32_kernel};
    void (*const kernel)(SIDE_ARGS) = kernels[p->mv_dtype];
    if (lds > 65536)             // (frames wider than 8192: one macroblock row is all a workgroup stages)
        HIPCHK(c, hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const size_t piece = 4 * es;
    L.mv_vec = mv_dst && gw % 4 == 0 && (uintptr_t)mv_dst % piece == 0 && mv_stride % piece == 0;
    L.info_vec = info_dst && gw % 4 == 0 && (uintptr_t)info_dst % 4 == 0 && info_stride % 4 == 0;
    if (!info_dst) L.planes = 0;             // (no info tensor: a cell makes none of its values)
    const unsigned groups = (unsigned)((L.mb_rows + L.R - 1) / L.R);
    for (int i0 = 0; i0 < n; i0 += SIDE_MAX_FRAMES) {
        const int m = n - i0 < SIDE_MAX_FRAMES ? n - i0 : SIDE_MAX_FRAMES;
        for (int k = 0; k < m; k++) {
            L.slot[k] = slots[i0 + k];
            L.q[k] = vp8hip_side_header_bits(c->slots[slots[i0 + k]].hdr_copy);
        }
        hipLaunchKernelGGL(kernel, dim3(groups * (unsigned)L.S, (unsigned)m), dim3(256), (unsigned)lds, c->stream, (const char *)c->slot_block_dev,
                           c->slot_bytes, c->o_mbx, c->o_mvs, mv_dst ? (uint8_t *)mv_dst + mv_stride * (size_t)i0 : (uint8_t *)nullptr, mv_stride,
                           info_dst ? (uint8_t *)info_dst + info_stride * (size_t)i0 : (uint8_t *)nullptr, info_stride, L);
        HIPCHK(c, hipGetLastError());
    }
    return 0;
}
