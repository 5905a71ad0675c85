// vp8hip_frames_trace_async, vp8hip_trace_flow_async, vp8hip_trace_residual_async, vp8hip_trace_gather_async, the trace's wear,
// vp8hip_frames_wear_async and vp8hip_trace_wear_async, and its inverse, vp8hip_trace_invert_async and vp8hip_trace_cover_async
// (include/vp8hip.h):
// accumulated motion -- every pixel traced back through the frames it was predicted from to the key frame that started the group -- in
// a pool in the caller's device memory, a pool entry as a flow tensor, a frame minus its anchor picture gathered at its trace as a
// residual tensor, and a tensor of the caller's gathered at a trace.  The plans and the checks are made here, once per call; the
// kernels are in vp8_trace.hip, vp8_trace_residual.hip, vp8_trace_gather.hip and vp8_trace_wear.hip (what happened to a pixel along its
// trace: four counters a pixel in a pool of its own, chained as the trace is, and a pool entry as a tensor) and vp8_trace_invert.hip
// (a trace scattered onto the anchor's grid: first descendant and descendant count per anchor pixel, and a count entry as a tensor).  The trace
// reads the slots' records and vectors (also on a vp8hip_configure_pooled context) and the pool entries its jobs name; the slots'
// header bits come with the launch, as of this call: nothing is allocated on the device, copied or synchronised.
#include "vp8hip_ctx.hip.h"

#define TRACE_ARGS const char *slot_base, size_t slot_bytes, size_t o_mbx, size_t o_mvs, uint8_t *pool, size_t pool_stride, TraceLaunch L
extern "C" __global__ void vp8_trace_kernel(TRACE_ARGS);
extern "C" __global__ void vp8_wear_kernel(TRACE_ARGS);
#define ENTRY_ARGS const uint8_t *pool, size_t pool_stride, uint8_t *dst, size_t dst_stride, EntryLaunch L
extern "C" __global__ void vp8_flow_i16_kernel(ENTRY_ARGS);
extern "C" __global__ void vp8_flow_f16_kernel(ENTRY_ARGS);
extern "C" __global__ void vp8_flow_f32_kernel(ENTRY_ARGS);
extern "C" __global__ void vp8_wear_u8_kernel(ENTRY_ARGS);
extern "C" __global__ void vp8_wear_f16_kernel(ENTRY_ARGS);
extern "C" __global__ void vp8_wear_f32_kernel(ENTRY_ARGS);
extern "C" __global__ void vp8_cover_u8_kernel(ENTRY_ARGS);
extern "C" __global__ void vp8_cover_f16_kernel(ENTRY_ARGS);
extern "C" __global__ void vp8_cover_f32_kernel(ENTRY_ARGS);
#define INVERT_FILL_ARGS uint8_t *first, size_t first_stride, uint8_t *count, size_t count_stride, InvertLaunch L
extern "C" __global__ void vp8_invert_fill_kernel(INVERT_FILL_ARGS);
#define INVERT_ARGS const uint8_t *pool, size_t pool_stride, uint8_t *first, size_t first_stride, uint8_t *count, size_t count_stride, InvertLaunch L
extern "C" __global__ void vp8_invert_first_kernel(INVERT_ARGS);
extern "C" __global__ void vp8_invert_count_kernel(INVERT_ARGS);
extern "C" __global__ void vp8_invert_both_kernel(INVERT_ARGS);

#define ANCHOR_ARGS const uint8_t *raster, size_t fb_stride, const uint8_t *tiles, size_t tile_frame, const uint8_t *pool, size_t pool_stride, \
                    uint8_t *dst, size_t dst_stride, AnchorLaunch L
extern "C" __global__ void vp8_anchor_i16_kernel(ANCHOR_ARGS);
extern "C" __global__ void vp8_anchor_f16_kernel(ANCHOR_ARGS);
extern "C" __global__ void vp8_anchor_f32_kernel(ANCHOR_ARGS);

#define GATHER_ARGS const uint8_t *pool, size_t pool_stride, const uint8_t *src, size_t src_stride, uint8_t *dst, size_t dst_stride, GatherLaunch L
extern "C" __global__ void vp8_gather_planar_nearest_1_kernel(GATHER_ARGS);
extern "C" __global__ void vp8_gather_planar_nearest_2_kernel(GATHER_ARGS);
extern "C" __global__ void vp8_gather_planar_nearest_4_kernel(GATHER_ARGS);
extern "C" __global__ void vp8_gather_rows_nearest_1_kernel(GATHER_ARGS);
extern "C" __global__ void vp8_gather_rows_nearest_2_kernel(GATHER_ARGS);
extern "C" __global__ void vp8_gather_rows_nearest_4_kernel(GATHER_ARGS);
extern "C" __global__ void vp8_gather_planar_bilinear_2_kernel(GATHER_ARGS);
extern "C" __global__ void vp8_gather_planar_bilinear_4_kernel(GATHER_ARGS);
extern "C" __global__ void vp8_gather_rows_bilinear_2_kernel(GATHER_ARGS);
extern "C" __global__ void vp8_gather_rows_bilinear_4_kernel(GATHER_ARGS);

#define TRACE_GROUP_LDS 32768                   // record dwords and vectors of a group of macroblock rows ...
#define TRACE_GROUP_ROWS 4                      // ... and at most this many rows
#define TRACE_MB_LDS 68                         // a macroblock in LDS: the record's first dword, sixteen vectors
#define FLOW_PART_QUADS 8192                    // groups of four outputs a workgroup of the flow kernel walks
#define ANCHOR_PART_QUADS 4096                  // ... and of the residual kernel: its loads wait on the trace's, so more waves in flight
#define GATHER_PART_QUADS 2048                  // ... and of the planar gather kernels, which make GATHER_GROUP_CH channels of each
#define GATHER_GROUP_CH 8                       // channels a workgroup of the planar gather kernels makes
#define INVERT_PART_QUADS 4096                  // groups of four trace pixels a workgroup of the fill and the scatter kernels walks

extern "C" size_t vp8hip_trace_size(const vp8hip_ctx *c) { return c && c->width ? (size_t)4 * c->width * c->height : 0; }

// the pool: pool_frames entries of the context's trace size, pool_stride apart, dword-aligned, inside one allocation of the device
// (that the entries a call names lie inside it is the call's to check: they sit in different structs and the texts differ)
int vp8hip_check_pool(vp8hip_ctx *c, const char *who, const void *pool, size_t pool_stride, int pool_frames)
{
    if (pool_frames < 1) return fail(c, -2, "%s: a pool of %d traces", who, pool_frames);
    return vp8hip_check_dst(c, who, pool, pool_stride, vp8hip_trace_size(c), 4, pool_frames);
}

// What vp8hip_frames_trace_async and vp8hip_frames_wear_async are: the checks of a call whose jobs chain entries of a pool through
// the slots' records and vectors, and the launches of `kernel` (vp8_trace_kernel's shape: groups of macroblock rows x jobs).
// who_pool: the name the pool's check speaks under
static int trace_frames(vp8hip_ctx *c, const char *who, const char *who_pool, void (*kernel)(TRACE_ARGS), const vp8hip_job *jobs, int n, void *pool,
                        size_t pool_stride, int pool_frames)
{
    if (!c || !jobs || n < 1 || !pool || c->slots.empty() || !c->width) return fail(c, -2, "%s: bad arguments", who);
    std::vector<int> slots((size_t)n);
    for (int i = 0; i < n; i++) slots[(size_t)i] = jobs[i].ir_slot;
    if (int rc = vp8hip_check_slots(c, who, slots.data(), n)) return rc;
    if (int rc = vp8hip_check_pool(c, who_pool, pool, pool_stride, pool_frames)) return rc;
    // one marker byte per pool entry: 1 a reference of some job, 2 some job's destination
    std::vector<uint8_t> mark((size_t)pool_frames, 0);
    for (int i = 0; i < n; i++) {
        if (jobs[i].dst_fb < 0 || jobs[i].dst_fb >= pool_frames) return fail(c, -2, "%s: job %d: destination %d outside the pool", who, i, jobs[i].dst_fb);
        for (int r = 1; r < 4; r++) {
            const int e = jobs[i].ref_fb[r];
            if (e < -1 || e >= pool_frames) return fail(c, -2, "%s: job %d: reference %d outside the pool", who, i, e);
            if (e >= 0) mark[(size_t)e] |= 1;
        }
    }
    for (int i = 0; i < n; i++) {
        uint8_t &m = mark[(size_t)jobs[i].dst_fb];
        if (m) return fail(c, -2, "%s: job %d: destination %d is %s of the call", who, i, jobs[i].dst_fb, m & 1 ? "a reference" : "another job's destination");
        m = 2;
    }
    HIPCHK(c, hipSetDevice(c->device));

    TraceLaunch L;
    memset(&L, 0, offsetof(TraceLaunch, j));
    L.dw = c->width; L.dh = c->height;
    L.mb_cols = c->dg.mb_cols; L.mb_rows = c->dg.mb_rows;
    const size_t row_bytes = (size_t)L.mb_cols * TRACE_MB_LDS;
    int R = (int)(TRACE_GROUP_LDS / row_bytes);
    R = R < 1 ? 1 : R > TRACE_GROUP_ROWS ? TRACE_GROUP_ROWS : R;
    if (R > L.mb_rows) R = L.mb_rows;
    L.R = R;
    const size_t lds = align_up((size_t)R * row_bytes, 16);
    if (lds > 65536)             // (frames wider than 15408: one macroblock row is all a workgroup stages)
        HIPCHK(c, hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    L.vec = L.dw % 4 == 0 && (uintptr_t)pool % 16 == 0 && pool_stride % 16 == 0;
    const unsigned groups = (unsigned)((L.mb_rows + R - 1) / R);
    for (int i0 = 0; i0 < n; i0 += TRACE_MAX_FRAMES) {
        const int m = n - i0 < TRACE_MAX_FRAMES ? n - i0 : TRACE_MAX_FRAMES;
        for (int k = 0; k < m; k++) {
            const vp8hip_job &job = jobs[i0 + k];
            TraceJob &J = L.j[k];
            J.slot = job.ir_slot; J.dst = job.dst_fb;
            J.ref[0] = job.ref_fb[1]; J.ref[1] = job.ref_fb[2]; J.ref[2] = job.ref_fb[3];
            J.key = c->slots[(size_t)job.ir_slot].hdr_copy.frame_type == 0;
        }
        hipLaunchKernelGGL(kernel, dim3(groups, (unsigned)m), dim3(256), (unsigned)lds, c->stream, (const char *)c->slot_block_dev,
                           c->slot_bytes, c->o_mbx, c->o_mvs, (uint8_t *)pool, pool_stride, L);
        HIPCHK(c, hipGetLastError());
    }
    return 0;
}

extern "C" int vp8hip_frames_trace_async(vp8hip_ctx *c, const vp8hip_job *jobs, int n, void *pool, size_t pool_stride, int pool_frames)
{
    return trace_frames(c, "vp8hip_frames_trace_async", "vp8hip_frames_trace_async (pool)", vp8_trace_kernel, jobs, n, pool, pool_stride, pool_frames);
}

// a wear entry has a trace's shape and size, and a macroblock takes the trace's 68 bytes of LDS (one dword of its record, sixteen vectors)
extern "C" int vp8hip_frames_wear_async(vp8hip_ctx *c, const vp8hip_job *jobs, int n, void *pool, size_t pool_stride, int pool_frames)
{
    return trace_frames(c, "vp8hip_frames_wear_async", "vp8hip_frames_wear_async (pool)", vp8_wear_kernel, jobs, n, pool, pool_stride, pool_frames);
}

// the grid of dst_w x dst_h on context c (null: sized grids only); false for what the calls refuse
static bool trace_out_grid(const vp8hip_ctx *c, int dst_w, int dst_h, int &gw, int &gh)
{
    if (dst_w == 0 && dst_h == 0) {              // the display size: the trace's own grid
        if (!c || !c->width) return false;
        gw = c->width; gh = c->height;
        return true;
    }
    return vp8hip_out_grid(c, dst_w, dst_h, 16, gw, gh);
}

// What the three readers' plans share: the grid gw x gh laid over the display size and shared by workgroups of part_quads groups of
// four outputs each, and whether the tensors at dst, dst_stride apart, of elements of es bytes take every group as one aligned piece
static TraceGrid trace_grid(const vp8hip_ctx *c, int gw, int gh, size_t es, int part_quads, const void *dst, size_t dst_stride)
{
    TraceGrid G;
    G.gw = gw; G.gh = gh; G.dw = c->width; G.dh = c->height;
    const long long quads = (long long)((gw + 3) >> 2) * gh;
    G.S = (int)((quads + part_quads - 1) / part_quads);
    if (G.S > gh) G.S = gh;
    G.xmode = gw == c->width ? SIDE_X_DISPLAY : SIDE_X_ANY;
    const size_t piece = 4 * es;
    G.vec = gw % 4 == 0 && (uintptr_t)dst % piece == 0 && dst_stride % piece == 0;
    return G;
}

// What vp8hip_trace_flow_async, vp8hip_trace_wear_async and vp8hip_trace_cover_async are: pool entries handed out as tensors
// (entry_tensor_body, vp8_trace_read.hip.h).  A call says what differs, and what its parameter struct holds (null: has_p false)
struct EntryCall {
    const char *who;              // the call's name
    const char *pool_name;        // the pool's name in messages
    int family;                   // the element of dtype 0, for vp8hip_elem_size: 2 (int16) or 1 (bytes)
    unsigned valid;               // the plane bits there are; 0: no choice, two planes always
    void (*kernels[3])(ENTRY_ARGS);
    bool has_p;
    int dst_w, dst_h, dtype;
    unsigned planes;
    float scale[4];
};

template <class P>
static EntryCall entry_call(EntryCall d, const P *p, unsigned planes, int nscale)
{
    d.has_p = true;
    d.dst_w = p->dst_w; d.dst_h = p->dst_h; d.dtype = p->dtype;
    d.planes = planes;
    for (int k = 0; k < nscale; k++) d.scale[k] = p->scale[k];
    return d;
}

// the grid of d on context c; false for what the call refuses on its parameters alone
static bool entry_grid(const vp8hip_ctx *c, const EntryCall &d, int &gw, int &gh)
{
    return d.has_p && d.dtype >= 0 && d.dtype <= 2 && (!d.valid || (d.planes && !(d.planes & ~d.valid))) && trace_out_grid(c, d.dst_w, d.dst_h, gw, gh);
}

// the bytes of one tensor on a grid of gw x gh
static size_t entry_bytes(const EntryCall &d, int gw, int gh)
{
    return (size_t)(d.valid ? __builtin_popcount(d.planes) : 2) * gh * gw * vp8hip_elem_size(d.dtype, d.family);
}

static size_t entry_size(const vp8hip_ctx *c, const EntryCall &d)
{
    int gw, gh;
    return entry_grid(c, d, gw, gh) ? entry_bytes(d, gw, gh) : 0;
}

static int entry_tensors(vp8hip_ctx *c, const EntryCall &d, const int *idx, int n, const void *pool, size_t pool_stride, int pool_frames, void *dst,
                         size_t dst_stride)
{
    const char *who = d.who;
    if (!c || !idx || n < 1 || !d.has_p || !pool || !dst || !c->width) return fail(c, -2, "%s: bad arguments", who);
    int gw, gh;
    if (!entry_grid(c, d, gw, gh)) {
        if (!d.valid) return fail(c, -2, "%s: grid %dx%d (both 0, or 1..%d each), type %d", who, d.dst_w, d.dst_h, VP8HIP_MAX_OUT_SIZE, d.dtype);
        return fail(c, -2, "%s: grid %dx%d (both 0, or 1..%d each), type %d, planes 0x%x", who, d.dst_w, d.dst_h, VP8HIP_MAX_OUT_SIZE, d.dtype, d.planes);
    }
    char who_pool[64], who_dst[64];
    snprintf(who_pool, sizeof(who_pool), "%s (%s)", who, d.pool_name);
    snprintf(who_dst, sizeof(who_dst), "%s (dst)", who);
    if (int rc = vp8hip_check_pool(c, who_pool, pool, pool_stride, pool_frames)) return rc;
    for (int i = 0; i < n; i++)
        if (idx[i] < 0 || idx[i] >= pool_frames) return fail(c, -2, "%s: entry %d outside the pool", who, idx[i]);
    const size_t es = (size_t)vp8hip_elem_size(d.dtype, d.family);
    if (int rc = vp8hip_check_dst(c, who_dst, dst, dst_stride, entry_bytes(d, gw, gh), es, n)) return rc;
    HIPCHK(c, hipSetDevice(c->device));

    EntryLaunch L;
    memset(&L, 0, offsetof(EntryLaunch, idx));
    L.g = trace_grid(c, gw, gh, es, FLOW_PART_QUADS, dst, dst_stride);
    L.planes = d.planes;
    for (int k = 0; k < 4; k++) L.scale[k] = d.scale[k];
    for (int i0 = 0; i0 < n; i0 += FLOW_MAX_FRAMES) {
        const int m = n - i0 < FLOW_MAX_FRAMES ? n - i0 : FLOW_MAX_FRAMES;
        memcpy(L.idx, idx + i0, sizeof(int) * (size_t)m);
        hipLaunchKernelGGL(d.kernels[d.dtype], dim3((unsigned)L.g.S, (unsigned)m), dim3(256), 0, c->stream, (const uint8_t *)pool, pool_stride,
                           (uint8_t *)dst + dst_stride * (size_t)i0, dst_stride, L);
        HIPCHK(c, hipGetLastError());
    }
    return 0;
}

static EntryCall flow_call(const vp8hip_trace_flow *p)
{
    const EntryCall d = {"vp8hip_trace_flow_async", "pool", 2, 0, {vp8_flow_i16_kernel, vp8_flow_f16_kernel, vp8_flow_f32_kernel}};
    return p ? entry_call(d, p, 0, 2) : d;
}

extern "C" size_t vp8hip_trace_flow_size(const vp8hip_ctx *c, const vp8hip_trace_flow *p) { return entry_size(c, flow_call(p)); }

extern "C" int vp8hip_trace_flow_async(vp8hip_ctx *c, const int *idx, int n, const vp8hip_trace_flow *p, const void *pool, size_t pool_stride,
                                       int pool_frames, void *dst, size_t dst_stride)
{
    return entry_tensors(c, flow_call(p), idx, n, pool, pool_stride, pool_frames, dst, dst_stride);
}

static EntryCall wear_call(const vp8hip_trace_wear *p)
{
    const EntryCall d = {"vp8hip_trace_wear_async", "pool", 1, VP8HIP_WEAR_HOPS | VP8HIP_WEAR_INTRA | VP8HIP_WEAR_EDGE | VP8HIP_WEAR_CODED,
                         {vp8_wear_u8_kernel, vp8_wear_f16_kernel, vp8_wear_f32_kernel}};
    return p ? entry_call(d, p, p->planes, 4) : d;
}

extern "C" size_t vp8hip_trace_wear_size(const vp8hip_ctx *c, const vp8hip_trace_wear *p) { return entry_size(c, wear_call(p)); }

extern "C" int vp8hip_trace_wear_async(vp8hip_ctx *c, const int *idx, int n, const vp8hip_trace_wear *p, const void *pool, size_t pool_stride,
                                       int pool_frames, void *dst, size_t dst_stride)
{
    return entry_tensors(c, wear_call(p), idx, n, pool, pool_stride, pool_frames, dst, dst_stride);
}

// [p, + stride * frames) and [q, + qstride * qframes) overlap -- what vp8hip_trace_invert_async refuses of its pools and
// vp8hip_trace_gather_async of src / dst: the span checks have bounded the products, so neither wraps, and the ends saturate
bool vp8hip_spans_overlap(const void *p, size_t stride, int frames, const void *q, size_t qstride, int qframes)
{
    const uintptr_t p0 = (uintptr_t)p, q0 = (uintptr_t)q;
    const size_t plen = stride * (size_t)frames, qlen = qstride * (size_t)qframes;
    const uintptr_t p1 = p0 + plen < p0 ? UINTPTR_MAX : p0 + plen, q1 = q0 + qlen < q0 ? UINTPTR_MAX : q0 + qlen;
    return p0 < q1 && q0 < p1;
}

extern "C" int vp8hip_trace_invert_async(vp8hip_ctx *c, const vp8hip_invert_job *jobs, int n, const void *pool, size_t pool_stride, int pool_frames,
                                         void *first, size_t first_stride, void *count, size_t count_stride, int out_frames)
{
    const char *who = "vp8hip_trace_invert_async";
    if (!c || !jobs || n < 1 || !pool || !c->width) return fail(c, -2, "%s: bad arguments", who);
    if (!first && !count) return fail(c, -2, "%s: neither a FIRST nor a COUNT pool", who);
    if (int rc = vp8hip_check_pool(c, "vp8hip_trace_invert_async (pool)", pool, pool_stride, pool_frames)) return rc;
    if (first)
        if (int rc = vp8hip_check_pool(c, "vp8hip_trace_invert_async (first)", first, first_stride, out_frames)) return rc;
    if (count)
        if (int rc = vp8hip_check_pool(c, "vp8hip_trace_invert_async (count)", count, count_stride, out_frames)) return rc;
    std::vector<uint8_t> mark((size_t)out_frames, 0);        // 1: some job's destination
    for (int i = 0; i < n; i++) {
        if (jobs[i].trace < 0 || jobs[i].trace >= pool_frames) return fail(c, -2, "%s: job %d: trace %d outside the pool", who, i, jobs[i].trace);
        if (jobs[i].dst < 0 || jobs[i].dst >= out_frames) return fail(c, -2, "%s: job %d: destination %d outside the pools", who, i, jobs[i].dst);
        uint8_t &m = mark[(size_t)jobs[i].dst];
        if (m) return fail(c, -2, "%s: job %d: destination %d is another job's destination", who, i, jobs[i].dst);
        m = 1;
    }
    if (first && vp8hip_spans_overlap(pool, pool_stride, pool_frames, first, first_stride, out_frames))
        return fail(c, -2, "%s: the trace pool and the FIRST pool overlap", who);
    if (count && vp8hip_spans_overlap(pool, pool_stride, pool_frames, count, count_stride, out_frames))
        return fail(c, -2, "%s: the trace pool and the COUNT pool overlap", who);
    if (first && count && vp8hip_spans_overlap(first, first_stride, out_frames, count, count_stride, out_frames))
        return fail(c, -2, "%s: the FIRST pool and the COUNT pool overlap", who);
    HIPCHK(c, hipSetDevice(c->device));

    InvertLaunch L;
    memset(&L, 0, offsetof(InvertLaunch, j));
    L.dw = c->width; L.dh = c->height;
    const long long quads = (long long)((L.dw + 3) >> 2) * L.dh;
    L.S = (int)((quads + INVERT_PART_QUADS - 1) / INVERT_PART_QUADS);
    if (L.S > L.dh) L.S = L.dh;
    L.vec = L.dw % 4 == 0 && (uintptr_t)pool % 16 == 0 && pool_stride % 16 == 0;
    L.first_vec = first && (uintptr_t)first % 16 == 0 && first_stride % 16 == 0;
    L.count_vec = count && (uintptr_t)count % 16 == 0 && count_stride % 16 == 0;
    void (*const kernel)(INVERT_ARGS) = !count ? vp8_invert_first_kernel : !first ? vp8_invert_count_kernel : vp8_invert_both_kernel;
    for (int i0 = 0; i0 < n; i0 += INVERT_MAX_JOBS) {
        const int m = n - i0 < INVERT_MAX_JOBS ? n - i0 : INVERT_MAX_JOBS;
        for (int k = 0; k < m; k++) {
            L.j[k].trace = jobs[i0 + k].trace;
            L.j[k].dst = jobs[i0 + k].dst;
        }
        // the fill, and behind it on the stream the scatter into what it wrote
        hipLaunchKernelGGL(vp8_invert_fill_kernel, dim3((unsigned)L.S, (unsigned)m), dim3(256), 0, c->stream, (uint8_t *)first, first_stride,
                           (uint8_t *)count, count_stride, L);
        HIPCHK(c, hipGetLastError());
        hipLaunchKernelGGL(kernel, dim3((unsigned)L.S, (unsigned)m), dim3(256), 0, c->stream, (const uint8_t *)pool, pool_stride, (uint8_t *)first,
                           first_stride, (uint8_t *)count, count_stride, L);
        HIPCHK(c, hipGetLastError());
    }
    return 0;
}

static EntryCall cover_call(const vp8hip_trace_cover *p)
{
    const EntryCall d = {"vp8hip_trace_cover_async", "count", 1, VP8HIP_COVER_COUNT | VP8HIP_COVER_SEEN,
                         {vp8_cover_u8_kernel, vp8_cover_f16_kernel, vp8_cover_f32_kernel}};
    return p ? entry_call(d, p, p->planes, 2) : d;
}

extern "C" size_t vp8hip_trace_cover_size(const vp8hip_ctx *c, const vp8hip_trace_cover *p) { return entry_size(c, cover_call(p)); }

extern "C" int vp8hip_trace_cover_async(vp8hip_ctx *c, const int *idx, int n, const vp8hip_trace_cover *p, const void *count, size_t count_stride,
                                        int count_frames, void *dst, size_t dst_stride)
{
    return entry_tensors(c, cover_call(p), idx, n, count, count_stride, count_frames, dst, dst_stride);
}

// the grid of p on context c; false for what the call refuses on p alone
static bool anchor_grid(const vp8hip_ctx *c, const vp8hip_trace_residual *p, int &gw, int &gh)
{
    return p && p->dtype >= 0 && p->dtype <= 2 && p->matrix >= 0 && p->matrix <= 2 && p->order >= 0 && p->order <= 1 &&
           trace_out_grid(c, p->dst_w, p->dst_h, gw, gh);
}

extern "C" size_t vp8hip_trace_residual_size(const vp8hip_ctx *c, const vp8hip_trace_residual *p)
{
    int gw, gh;
    return anchor_grid(c, p, gw, gh) ? (size_t)3 * gh * gw * vp8hip_elem_size(p->dtype, 2) : 0;
}

extern "C" int vp8hip_trace_residual_async(vp8hip_ctx *c, const vp8hip_anchor_job *jobs, int n, const vp8hip_trace_residual *p, const void *pool,
                                           size_t pool_stride, int pool_frames, void *dst, size_t dst_stride)
{
    const char *who = "vp8hip_trace_residual_async";
    if (!c || !jobs || n < 1 || !p || !pool || !dst || !c->width || c->fb.empty()) return fail(c, -2, "%s: bad arguments", who);
    for (int i = 0; i < n; i++) {
        const int fbs[2] = {jobs[i].fb, jobs[i].anchor_fb};
        if (int rc = vp8hip_check_fbs(c, who, fbs, 2)) return rc;
    }
    int gw, gh;
    if (!anchor_grid(c, p, gw, gh))
        return fail(c, -2, "%s: grid %dx%d (both 0, or 1..%d each), matrix %d, order %d, type %d", who, p->dst_w, p->dst_h, VP8HIP_MAX_OUT_SIZE,
                    p->matrix, p->order, p->dtype);
    if (int rc = vp8hip_check_pool(c, "vp8hip_trace_residual_async (pool)", pool, pool_stride, pool_frames)) return rc;
    for (int i = 0; i < n; i++)
        if (jobs[i].trace < 0 || jobs[i].trace >= pool_frames) return fail(c, -2, "%s: job %d: trace %d outside the pool", who, i, jobs[i].trace);
    const size_t es = (size_t)vp8hip_elem_size(p->dtype, 2);
    const size_t size = (size_t)3 * gh * gw * es;
    if (int rc = vp8hip_check_dst(c, "vp8hip_trace_residual_async (dst)", dst, dst_stride, size, es, n)) return rc;
    HIPCHK(c, hipSetDevice(c->device));

    AnchorLaunch L;
    memset(&L, 0, offsetof(AnchorLaunch, j));
    L.g = trace_grid(c, gw, gh, es, ANCHOR_PART_QUADS, dst, dst_stride);
    L.mb_cols = c->dg.mb_cols;
    L.aw = c->dg.aligned_w; L.ah = c->dg.aligned_h;
    L.y_off = c->dg.y_off; L.u_off = c->dg.u_off; L.v_off = c->dg.v_off;
    L.y_stride = c->dg.y_stride; L.uv_stride = c->dg.uv_stride;
    vp8hip_rgb_coeffs(p->matrix, p->order, L.cy, L.k0, L.cu, L.cv);
    for (int pos = 0; pos < 3; pos++) L.scale[pos] = p->scale[p->order ? 2 - pos : pos];
    void (*const kernels[3])(ANCHOR_ARGS) = {vp8_anchor_i16_kernel, vp8_anchor_f16_kernel, vp8_anchor_f32_kernel};
    for (int i0 = 0; i0 < n; i0 += ANCHOR_MAX_FRAMES) {
        const int m = n - i0 < ANCHOR_MAX_FRAMES ? n - i0 : ANCHOR_MAX_FRAMES;
        for (int k = 0; k < m; k++) {
            const vp8hip_anchor_job &job = jobs[i0 + k];
            // each frame buffer in a form it has: raster where it exists, else tiles; the two of a job independently
            L.j[k].fb = vp8hip_frame_ref(c, job.fb);
            L.j[k].trace = job.trace;
            L.j[k].anchor = vp8hip_frame_ref(c, job.anchor_fb);
        }
        hipLaunchKernelGGL(kernels[p->dtype], dim3((unsigned)L.g.S, (unsigned)m), dim3(256), 0, c->stream, (const uint8_t *)c->fb_block, c->fb_stride,
                           (const uint8_t *)c->tile_block, c->tile_frame, (const uint8_t *)pool, pool_stride,
                           (uint8_t *)dst + dst_stride * (size_t)i0, dst_stride, L);
        HIPCHK(c, hipGetLastError());
    }
    return 0;
}

// the grids of p on context c; false for what the call refuses on p alone
static bool gather_grid(const vp8hip_ctx *c, const vp8hip_trace_gather *p, int &gw, int &gh)
{
    return p && p->src_w >= 1 && p->src_w <= VP8HIP_MAX_OUT_SIZE && p->src_h >= 1 && p->src_h <= VP8HIP_MAX_OUT_SIZE && p->channels >= 1 &&
           p->channels <= VP8HIP_GATHER_MAX_CHANNELS && (p->elem == 1 || p->elem == 2 || p->elem == 4) &&
           (p->layout == VP8HIP_GATHER_PLANAR || p->layout == VP8HIP_GATHER_CHANNELS_LAST) &&
           (p->filter == VP8HIP_GATHER_NEAREST || (p->filter == VP8HIP_GATHER_BILINEAR && p->elem != 1)) &&
           trace_out_grid(c, p->dst_w, p->dst_h, gw, gh);
}

extern "C" size_t vp8hip_trace_gather_size(const vp8hip_ctx *c, const vp8hip_trace_gather *p)
{
    int gw, gh;
    return gather_grid(c, p, gw, gh) ? (size_t)p->channels * gh * gw * (size_t)p->elem : 0;
}

extern "C" int vp8hip_trace_gather_async(vp8hip_ctx *c, const vp8hip_gather_job *jobs, int n, const vp8hip_trace_gather *p, const void *pool,
                                         size_t pool_stride, int pool_frames, const void *src, size_t src_stride, int src_frames, void *dst,
                                         size_t dst_stride)
{
    const char *who = "vp8hip_trace_gather_async";
    if (!c || !jobs || n < 1 || !p || !pool || !src || !dst || !c->width) return fail(c, -2, "%s: bad arguments", who);
    int gw, gh;
    if (!gather_grid(c, p, gw, gh))
        return fail(c, -2, "%s: grid %dx%d (both 0, or 1..%d each), source grid %dx%d (1..%d each), %d channels (1..%d), element %d, layout %d, filter %d",
                    who, p->dst_w, p->dst_h, VP8HIP_MAX_OUT_SIZE, p->src_w, p->src_h, VP8HIP_MAX_OUT_SIZE, p->channels, VP8HIP_GATHER_MAX_CHANNELS,
                    p->elem, p->layout, p->filter);
    if (int rc = vp8hip_check_pool(c, "vp8hip_trace_gather_async (pool)", pool, pool_stride, pool_frames)) return rc;
    if (src_frames < 1) return fail(c, -2, "%s: %d source tensors", who, src_frames);
    for (int i = 0; i < n; i++) {
        if (jobs[i].trace < 0 || jobs[i].trace >= pool_frames) return fail(c, -2, "%s: job %d: trace %d outside the pool", who, i, jobs[i].trace);
        if (jobs[i].src < 0 || jobs[i].src >= src_frames) return fail(c, -2, "%s: job %d: source tensor %d out of range", who, i, jobs[i].src);
    }
    const size_t es = (size_t)p->elem;
    const size_t ssize = (size_t)p->channels * p->src_h * p->src_w * es, size = (size_t)p->channels * gh * gw * es;
    if (int rc = vp8hip_check_dst(c, "vp8hip_trace_gather_async (src)", src, src_stride, ssize, es, src_frames)) return rc;
    if (int rc = vp8hip_check_dst(c, "vp8hip_trace_gather_async (dst)", dst, dst_stride, size, es, n)) return rc;
    if (vp8hip_spans_overlap(src, src_stride, src_frames, dst, dst_stride, n)) return fail(c, -2, "%s: the source tensors and the destination overlap", who);
    HIPCHK(c, hipSetDevice(c->device));

    GatherLaunch L;
    memset(&L, 0, offsetof(GatherLaunch, j));
    L.g = trace_grid(c, gw, gh, es, GATHER_PART_QUADS, dst, dst_stride);
    L.sw = p->src_w; L.sh = p->src_h;
    L.C = p->channels;
    unsigned gz = 1;
    if (p->layout == VP8HIP_GATHER_PLANAR) {
        L.cgroup = GATHER_GROUP_CH;
        gz = (unsigned)((L.C + L.cgroup - 1) / L.cgroup);
    } else {
        L.g.S = (int)(((long long)gw * gh + GATHER_RUN - 1) / GATHER_RUN);
        L.g.vec = ((size_t)L.C * es) % 16 == 0 && (uintptr_t)dst % 16 == 0 && dst_stride % 16 == 0 && (uintptr_t)src % 16 == 0 && src_stride % 16 == 0;
    }
    // by filter, layout and element size (1, 2, 4)
    void (*const kernels[2][2][3])(GATHER_ARGS) = {
        {{vp8_gather_planar_nearest_1_kernel, vp8_gather_planar_nearest_2_kernel, vp8_gather_planar_nearest_4_kernel},
         {vp8_gather_rows_nearest_1_kernel, vp8_gather_rows_nearest_2_kernel, vp8_gather_rows_nearest_4_kernel}},
        {{nullptr, vp8_gather_planar_bilinear_2_kernel, vp8_gather_planar_bilinear_4_kernel},
         {nullptr, vp8_gather_rows_bilinear_2_kernel, vp8_gather_rows_bilinear_4_kernel}}};
    void (*const kernel)(GATHER_ARGS) = kernels[p->filter][p->layout][p->elem >> 1];
    for (int i0 = 0; i0 < n; i0 += GATHER_MAX_JOBS) {
        const int m = n - i0 < GATHER_MAX_JOBS ? n - i0 : GATHER_MAX_JOBS;
        for (int k = 0; k < m; k++) {
            L.j[k].trace = jobs[i0 + k].trace;
            L.j[k].src = jobs[i0 + k].src;
        }
        hipLaunchKernelGGL(kernel, dim3((unsigned)L.g.S, (unsigned)m, gz), dim3(256), 0, c->stream, (const uint8_t *)pool, pool_stride,
                           (const uint8_t *)src, src_stride, (uint8_t *)dst + dst_stride * (size_t)i0, dst_stride, L);
        HIPCHK(c, hipGetLastError());
    }
    return 0;
}
