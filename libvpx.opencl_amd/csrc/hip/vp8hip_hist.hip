// vp8hip_frames_hist_async, vp8hip_slots_hist_async, vp8hip_trace_wear_hist_async and vp8hip_trace_cover_hist_async
// (include/vp8hip.h): byte histograms of pictures and picture pairs, of the slots' info planes on the native grid and of wear and
// COUNT entries, [planes][256] uint32 per job in the caller's device memory.  The plans and the checks are made here, once per call;
// the kernels are in vp8_hist.hip.  Everything they read is in the frame buffers as they lie (either form, nothing converted), in
// the slots (records and vectors: also on a vp8hip_configure_pooled context), in the caller's pool, or comes with the launch:
// nothing is allocated on the device, copied or synchronised.
#include "vp8hip_ctx.hip.h"

extern "C" __global__ void vp8_hist_fill_kernel(uint8_t *dst, size_t dst_stride, int dwords);
extern "C" __global__ void vp8_hist_frames_kernel(const uint8_t *raster, size_t fb_stride, const uint8_t *tiles, size_t tile_frame, uint8_t *dst,
                                                  size_t dst_stride, HistFrameLaunch L);
extern "C" __global__ void vp8_hist_slots_kernel(const char *slot_base, size_t slot_bytes, size_t o_mbx, size_t o_mvs, uint8_t *dst,
                                                 size_t dst_stride, HistSlotLaunch L);
#define HIST_ENTRY_ARGS const uint8_t *pool, size_t pool_stride, uint8_t *dst, size_t dst_stride, HistEntryLaunch L
extern "C" __global__ void vp8_hist_wear_kernel(HIST_ENTRY_ARGS);
extern "C" __global__ void vp8_hist_cover_kernel(HIST_ENTRY_ARGS);

#define HIST_CHIP_WGS 2048                      // workgroups a call aims at: calls of fewer jobs share a job among several ...
#define HIST_PART_QUADS 1024                    // ... of at least this many groups of 16 bytes each (four a lane)
#define HIST_GROUP_LDS 32768                    // records and vectors of a group of macroblock rows (vp8hip_side.hip's) ...
#define HIST_GROUP_ROWS 4                       // ... and at most this many rows
#define HIST_SLOT_COPIES 4                      // sub-histograms a plane in LDS: vp8_hist.hip's 4 * HIST_SLOT_LREP ...
#define HIST_ENTRY_COPIES 8                     // ... and 4 * HIST_ENTRY_LREP

extern "C" size_t vp8hip_hist_size(int planes_popcount)
{
    return planes_popcount >= 1 && planes_popcount <= 32 ? (size_t)planes_popcount * HIST_BINS * 4 : 0;
}

// what every call checks of its planes and its destination: np planes of `valid`, n outputs
static int hist_check_out(vp8hip_ctx *c, const char *who, unsigned planes, unsigned valid, void *dst, size_t dst_stride, int n)
{
    if (!planes || (planes & ~valid)) return fail(c, -2, "%s: planes 0x%x (at least one of 0x%x)", who, planes, valid);
    return vp8hip_check_named_dst(c, who, "dst", dst, dst_stride, vp8hip_hist_size(__builtin_popcount(planes)), 4, n);
}

// workgroups that share a job of `quads` groups in `rows` rows, in a call of n jobs
static int hist_share(int n, long long quads, int rows)
{
    long long S = (HIST_CHIP_WGS + n - 1) / n;
    const long long most = (quads + HIST_PART_QUADS - 1) / HIST_PART_QUADS;
    if (S > most) S = most;
    if (S > rows) S = rows;
    return S < 1 ? 1 : (int)S;
}

// the outputs of a launch of m jobs zeroed, where `wgs` workgroups will add to each
static int hist_fill(vp8hip_ctx *c, unsigned wgs, unsigned planes, uint8_t *dst, size_t dst_stride, int m)
{
    if (wgs < 2) return 0;
    const int np = __builtin_popcount(planes);
    hipLaunchKernelGGL(vp8_hist_fill_kernel, dim3((unsigned)np, (unsigned)m), dim3(256), 0, c->stream, dst, dst_stride, np * HIST_BINS);
    HIPCHK(c, hipGetLastError());
    return 0;
}

extern "C" int vp8hip_frames_hist_async(vp8hip_ctx *c, const vp8hip_hist_job *jobs, int n, unsigned planes, void *dst, size_t dst_stride)
{
    const char *who = "vp8hip_frames_hist_async";
    if (!c || !jobs || n < 1 || !dst || !c->width || c->fb.empty()) return fail(c, -2, "%s: bad arguments", who);
    if (int rc = vp8hip_check_pairs(c, who, jobs, n, true)) return rc;
    if (int rc = hist_check_out(c, who, planes, VP8HIP_HIST_YUV, dst, dst_stride, n)) return rc;
    HIPCHK(c, hipSetDevice(c->device));

    HistFrameLaunch L;
    memset(&L, 0, sizeof(L) - sizeof(L.j));
    vp8hip_frame_planes(c, L);
    L.S = hist_share(n, (long long)((L.dw + 15) >> 4) * L.dh, (L.dh + 1) >> 1);
    L.planes = planes;
    for (int i0 = 0; i0 < n; i0 += HIST_MAX_JOBS) {
        const int m = n - i0 < HIST_MAX_JOBS ? n - i0 : HIST_MAX_JOBS;
        for (int k = 0; k < m; k++) {
            const vp8hip_hist_job &job = jobs[i0 + k];
            L.j[k].fb = vp8hip_frame_ref(c, job.fb);
            L.j[k].ref = job.ref_fb < 0 ? -1 : vp8hip_frame_ref(c, job.ref_fb);
        }
        uint8_t *d = (uint8_t *)dst + dst_stride * (size_t)i0;
        if (int rc = hist_fill(c, (unsigned)L.S, planes, d, dst_stride, m)) return rc;
        hipLaunchKernelGGL(vp8_hist_frames_kernel, dim3((unsigned)L.S, (unsigned)m), dim3(256), 0, c->stream, (const uint8_t *)c->fb_block,
                           c->fb_stride, (const uint8_t *)c->tile_block, c->tile_frame, d, dst_stride, L);
        HIPCHK(c, hipGetLastError());
    }
    return 0;
}

extern "C" int vp8hip_slots_hist_async(vp8hip_ctx *c, const int *slots, int n, unsigned planes, void *dst, size_t dst_stride)
{
    const char *who = "vp8hip_slots_hist_async";
    if (!c || !slots || n < 1 || !dst || c->slots.empty()) return fail(c, -2, "%s: bad arguments", who);
    if (int rc = vp8hip_check_slots(c, who, slots, n)) return rc;
    const unsigned valid = VP8HIP_SIDE_REF | VP8HIP_SIDE_MODE | VP8HIP_SIDE_SKIP | VP8HIP_SIDE_SEGMENT | VP8HIP_SIDE_QINDEX | VP8HIP_SIDE_CODED |
                           VP8HIP_HIST_MVMAG;
    if (int rc = hist_check_out(c, who, planes, valid, dst, dst_stride, n)) return rc;
    HIPCHK(c, hipSetDevice(c->device));

    // the group of macroblock rows a workgroup stages: vp8hip_side.hip's
    HistSlotLaunch L;
    memset(&L, 0, offsetof(HistSlotLaunch, slot));
    L.mb_cols = c->dg.mb_cols; L.mb_rows = c->dg.mb_rows;
    const size_t row_bytes = (size_t)L.mb_cols * 128;
    int R = (int)(HIST_GROUP_LDS / row_bytes);
    R = R < 1 ? 1 : R > HIST_GROUP_ROWS ? HIST_GROUP_ROWS : R;
    if (R > L.mb_rows) R = L.mb_rows;
    L.R = R;
    L.planes = planes;
    const size_t hist_dwords = align_up((size_t)__builtin_popcount(planes) * HIST_SLOT_COPIES * HIST_ROW, 4);
    const size_t lds = hist_dwords * 4 + (size_t)R * row_bytes;
    if (lds > 65536)             // (frames wider than 4600 or so: one macroblock row is all a workgroup stages)
        HIPCHK(c, hipFuncSetAttribute((const void *)vp8_hist_slots_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const unsigned groups = (unsigned)((L.mb_rows + R - 1) / R);
    for (int i0 = 0; i0 < n; i0 += HIST_MAX_JOBS) {
        const int m = n - i0 < HIST_MAX_JOBS ? n - i0 : HIST_MAX_JOBS;
        for (int k = 0; k < m; k++) {
            L.slot[k] = slots[i0 + k];
            L.q[k] = vp8hip_side_header_bits(c->slots[(size_t)slots[i0 + k]].hdr_copy);
        }
        uint8_t *d = (uint8_t *)dst + dst_stride * (size_t)i0;
        if (int rc = hist_fill(c, groups, planes, d, dst_stride, m)) return rc;
        hipLaunchKernelGGL(vp8_hist_slots_kernel, dim3(groups, (unsigned)m), dim3(256), (unsigned)lds, c->stream, (const char *)c->slot_block_dev,
                           c->slot_bytes, c->o_mbx, c->o_mvs, d, dst_stride, L);
        HIPCHK(c, hipGetLastError());
    }
    return 0;
}

// What vp8hip_trace_wear_hist_async and vp8hip_trace_cover_hist_async are: the histograms of the planes `valid` has of pool entries
static int hist_entries(vp8hip_ctx *c, const char *who, const char *pool_name, unsigned valid, void (*kernel)(HIST_ENTRY_ARGS), const int *idx, int n,
                        unsigned planes, const void *pool, size_t pool_stride, int pool_frames, void *dst, size_t dst_stride)
{
    if (!c || !idx || n < 1 || !pool || !dst || !c->width) return fail(c, -2, "%s: bad arguments", who);
    char who_pool[64];
    snprintf(who_pool, sizeof(who_pool), "%s (%s)", who, pool_name);
    if (int rc = vp8hip_check_pool(c, who_pool, pool, pool_stride, pool_frames)) return rc;
    for (int i = 0; i < n; i++)
        if (idx[i] < 0 || idx[i] >= pool_frames) return fail(c, -2, "%s: entry %d outside the pool", who, idx[i]);
    if (int rc = hist_check_out(c, who, planes, valid, dst, dst_stride, n)) return rc;
    if (vp8hip_spans_overlap(dst, dst_stride, n, pool, pool_stride, pool_frames)) return fail(c, -2, "%s: the destination and the %s overlap", who, pool_name);
    HIPCHK(c, hipSetDevice(c->device));

    HistEntryLaunch L;
    memset(&L, 0, offsetof(HistEntryLaunch, idx));
    L.dw = c->width; L.dh = c->height;
    L.S = hist_share(n, ((long long)L.dw * L.dh + 3) >> 2, L.dh);
    L.planes = planes;
    const size_t lds = (size_t)__builtin_popcount(planes) * HIST_ENTRY_COPIES * HIST_ROW * 4;
    for (int i0 = 0; i0 < n; i0 += HIST_MAX_JOBS) {
        const int m = n - i0 < HIST_MAX_JOBS ? n - i0 : HIST_MAX_JOBS;
        memcpy(L.idx, idx + i0, sizeof(int) * (size_t)m);
        uint8_t *d = (uint8_t *)dst + dst_stride * (size_t)i0;
        if (int rc = hist_fill(c, (unsigned)L.S, planes, d, dst_stride, m)) return rc;
        hipLaunchKernelGGL(kernel, dim3((unsigned)L.S, (unsigned)m), dim3(256), (unsigned)lds, c->stream, (const uint8_t *)pool, pool_stride, d,
                           dst_stride, L);
        HIPCHK(c, hipGetLastError());
    }
    return 0;
}

extern "C" int vp8hip_trace_wear_hist_async(vp8hip_ctx *c, const int *idx, int n, unsigned planes, const void *pool, size_t pool_stride,
                                            int pool_frames, void *dst, size_t dst_stride)
{
    return hist_entries(c, "vp8hip_trace_wear_hist_async", "pool", VP8HIP_WEAR_HOPS | VP8HIP_WEAR_INTRA | VP8HIP_WEAR_EDGE | VP8HIP_WEAR_CODED,
                        vp8_hist_wear_kernel, idx, n, planes, pool, pool_stride, pool_frames, dst, dst_stride);
}

extern "C" int vp8hip_trace_cover_hist_async(vp8hip_ctx *c, const int *idx, int n, unsigned planes, const void *count, size_t count_stride,
                                             int count_frames, void *dst, size_t dst_stride)
{
    return hist_entries(c, "vp8hip_trace_cover_hist_async", "count", VP8HIP_COVER_COUNT | VP8HIP_COVER_SEEN, vp8_hist_cover_kernel, idx, n, planes,
                        count, count_stride, count_frames, dst, dst_stride);
}
