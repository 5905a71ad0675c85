// vp8hip_frames_coef_async (include/vp8hip.h): the transform coefficients of IR slots as tensors in the caller's device memory, and the
// host's vp8hip_dequant_factors.  The plan is made here, once per call; the kernels are in vp8_coef.hip.  Everything they read is in
// the slots (records and block stream; on a vp8hip_configure_pooled context the blocks lie in the pool) or comes with the launch (the
// slots' quantiser header as of this call): nothing is allocated, copied or synchronised.
#include "vp8hip_ctx.hip.h"

#define COEF_ARGS const char *slot_base, size_t slot_bytes, size_t o_mbx, size_t o_blocks, const char *pool, unsigned cap_blocks, uint8_t *dst, \
                  size_t dst_stride, CoefLaunch L
extern "C" __global__ void vp8_coef_i16_kernel(COEF_ARGS);
extern "C" __global__ void vp8_coef_f16_kernel(COEF_ARGS);
extern "C" __global__ void vp8_coef_f32_kernel(COEF_ARGS);

static_assert(sizeof(CoefLaunch) < 3072, "the kernel arguments stay well under 4 KB");
static_assert(VP8HIP_COEF_DEQUANT == COEF_DEQUANT && VP8HIP_COEF_LEVELS == COEF_LEVELS && VP8HIP_COEF_CHANNELS == COEF_CHANNELS &&
              VP8HIP_COEF_INPLACE == COEF_INPLACE, "the kernels' numbers are the header's");

// false for what the call refuses on p alone
static bool coef_params_ok(const vp8hip_coef *p)
{
    if (!p || p->dtype < 0 || p->dtype > 2) return false;
    if (p->stage != VP8HIP_COEF_DEQUANT && p->stage != VP8HIP_COEF_LEVELS) return false;
    if (p->layout != VP8HIP_COEF_CHANNELS && p->layout != VP8HIP_COEF_INPLACE) return false;
    if (p->order != VP8HIP_COEF_RASTER && p->order != VP8HIP_COEF_ZIGZAG) return false;
    if (p->nfreq < 1 || p->nfreq > 16) return false;
    if (p->layout == VP8HIP_COEF_INPLACE && (p->nfreq != 16 || p->order != VP8HIP_COEF_RASTER)) return false;
    const unsigned all = VP8HIP_COEF_Y | VP8HIP_COEF_U | VP8HIP_COEF_V | VP8HIP_COEF_Y2;
    return p->planes != 0 && !(p->planes & ~all);
}

// elements of plane k (Y, U, V, Y2) of a frame of cols x rows macroblocks: nfreq channels of G x G cells a macroblock, INPLACE: 16
static size_t coef_plane_elems(const vp8hip_coef *p, int k, int cols, int rows)
{
    const size_t G = k == 0 ? 4 : k == 3 ? 1 : 2;
    return (size_t)p->nfreq * G * rows * G * cols;
}

extern "C" size_t vp8hip_coef_size(const vp8hip_ctx *c, const vp8hip_coef *p)
{
    if (!c || !c->width || !coef_params_ok(p)) return 0;
    size_t elems = 0;
    for (int k = 0; k < COEF_PLANES; k++)
        if ((p->planes >> k) & 1u) elems += coef_plane_elems(p, k, c->dg.mb_cols, c->dg.mb_rows);
    return elems * vp8hip_elem_size(p->dtype, 2);
}

extern "C" int vp8hip_dequant_factors(const vp8ir_frame_hdr *h, int16_t out[4][6])
{
    static const unsigned short dc_q[128] = { VP8_DC_Q_VALUES }, ac_q[128] = { VP8_AC_Q_VALUES };
    if (!h || !out) return -2;
    const unsigned qbits = vp8hip_segment_q_bits(*h);
    for (int s = 0; s < 4; s++) {
        // vp8cx_init_de_quantizer + mb_init_dequantizer (decodframe.c:50-109), as res_macroblock (vp8_res_mb.hip.h)
        const int q = (int)((qbits >> (7 * s)) & 127u);
        auto qi = [q](int delta) { const int v = q + delta; return v < 0 ? 0 : v > 127 ? 127 : v; };
        int y2ac = (ac_q[qi(h->y2ac_delta_q)] * 155) / 100; if (y2ac < 8) y2ac = 8;
        int uvdc = dc_q[qi(h->uvdc_delta_q)]; if (uvdc > 132) uvdc = 132;
        out[s][0] = (int16_t)dc_q[qi(h->y1dc_delta_q)];
        out[s][1] = (int16_t)ac_q[q];
        out[s][2] = (int16_t)(dc_q[qi(h->y2dc_delta_q)] * 2);
        out[s][3] = (int16_t)y2ac;
        out[s][4] = (int16_t)uvdc;
        out[s][5] = (int16_t)ac_q[qi(h->uvac_delta_q)];
    }
    return 0;
}

extern "C" int vp8hip_frames_coef_async(vp8hip_ctx *c, const int *slots, int n, const vp8hip_coef *p, void *dst, size_t dst_stride)
{
    const char *who = "vp8hip_frames_coef_async";
    if (!c || !slots || n < 1 || !p || !dst || c->slots.empty()) return fail(c, -2, "%s: bad arguments", who);
    if (int rc = vp8hip_check_slots(c, who, slots, n)) return rc;
    const size_t size = vp8hip_coef_size(c, p);
    if (!size)
        return fail(c, -2, "%s: stage %d, layout %d, order %d, nfreq %d (1..16; in place: 16, raster), planes %#x, type %d", who, p->stage, p->layout,
                    p->order, p->nfreq, p->planes, p->dtype);
    const size_t es = (size_t)vp8hip_elem_size(p->dtype, 2);
    if (int rc = vp8hip_check_dst(c, who, dst, dst_stride, size, es, n)) return rc;
    HIPCHK(c, hipSetDevice(c->device));

    CoefLaunch L;
    memset(&L, 0, offsetof(CoefLaunch, s));
    L.mb_cols = c->dg.mb_cols; L.mb_rows = c->dg.mb_rows;
    L.runs = (L.mb_cols + COEF_RUN - 1) / COEF_RUN;
    L.stage = p->stage; L.layout = p->layout; L.zigzag = p->order == VP8HIP_COEF_ZIGZAG; L.nfreq = p->nfreq;
    L.planes = p->planes;
    const size_t piece = 4 * es;
    const bool aligned = (uintptr_t)dst % piece == 0 && dst_stride % piece == 0;
    size_t at = 0;
    for (int k = 0; k < COEF_PLANES; k++) {
        if (!((p->planes >> k) & 1u)) continue;
        // a row of the plane: G (in place: 4G) elements a macroblock.  (Every plane is a multiple of 4 elements but Y2's, the last.)
        const size_t row = (size_t)(k == 0 ? 4 : k == 3 ? 1 : 2) * (p->layout == VP8HIP_COEF_INPLACE ? 4 : 1) * L.mb_cols;
        L.off[k] = at;
        L.scale[k] = p->scale[k];
        if (aligned && row % 4 == 0 && at % 4 == 0) L.vec |= 1u << k;
        at += coef_plane_elems(p, k, L.mb_cols, L.mb_rows);
    }
    void (*const kernels[3])(COEF_ARGS) = {vp8_coef_i16_kernel, vp8_coef_f16_kernel, vp8_coef_f32_kernel};
    void (*const kernel)(COEF_ARGS) = kernels[p->dtype];
    const size_t cap = c->pool ? ((size_t)c->pool_chunks + 1) * c->chunk_blocks : c->cap_blocks;
    // (the kernel clamps a block's index to cap - 1, as 32 bits: what keeps a starved slot's reads in bounds)
    if (cap < 1 || cap > 0xffffffffull) return fail(c, -2, "%s: a block stream of %zu blocks", who, cap);
    const unsigned groups = (unsigned)(L.mb_rows * L.runs);
    for (int i0 = 0; i0 < n; i0 += RES_MAX_FRAMES) {
        const int m = n - i0 < RES_MAX_FRAMES ? n - i0 : RES_MAX_FRAMES;
        for (int k = 0; k < m; k++) L.s[k] = vp8hip_res_header_bits(slots[i0 + k], c->slots[slots[i0 + k]].hdr_copy);
        hipLaunchKernelGGL(kernel, dim3(groups, (unsigned)m), dim3(256), 0, c->stream, (const char *)c->slot_block_dev, c->slot_bytes, c->o_mbx,
                           c->o_blocks, (const char *)c->pool, (unsigned)cap, (uint8_t *)dst + dst_stride * (size_t)i0, dst_stride, L);
        HIPCHK(c, hipGetLastError());
    }
    return 0;
}
