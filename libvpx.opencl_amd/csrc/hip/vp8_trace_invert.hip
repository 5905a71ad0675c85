// A trace inverted (vp8hip_trace_invert_async and vp8hip_trace_cover_async, vp8hip_trace.hip; include/vp8hip.h has the definitions).
// A trace says where in the anchor picture a frame pixel descends from; the inverse says, for every pixel a of the ANCHOR's grid,
// which frame pixels name it: FIRST(a), the first of them in raster order packed as a trace packs a position (0xffffffff: none), and
// COUNT(a), how many there are.  Both are entries of pools of a trace pool's geometry in the caller's device memory.
//
// vp8_invert_fill_kernel writes the jobs' FIRST entries to 0xffffffff and their COUNT entries to 0: an entry is d_w * d_h dwords in a
// row, taken as whole 16-byte pieces where the pool allows and a tail of dwords, or dword by dword.
//
// vp8_invert_*_kernel, on the same stream behind it: for every pixel of the trace an unsigned atomic minimum of y << 16 | x on the
// FIRST dword and an atomic add of 1 on the COUNT dword of the anchor pixel the trace names.  Positions are below 16384, so the
// unsigned order of the packed dword is raster order and 0xffffffff is above every position; minimum and integer add do not care in
// what order lanes arrive, so two runs give the same bits.  The atomics' results are not used: they go out as vector global
// atomics without return.  One kernel per set of outputs, so that a call for one output issues only that output's atomics.
// THE LANE WALK: a wave takes a run of 256 pixels of the workgroup's rows as four instructions of 64 neighbouring pixels, a dword a
// lane.  The chip takes atomics at full rate where a wave instruction covers 256 contiguous bytes, and traces of block motion keep
// neighbours together, so this walk gives it that shape.  With -DINVERT_LANE_QUADS a lane takes four neighbouring pixels of a row
// instead (one 16-byte load where InvertLaunch::vec, else the dwords that exist, each once), as the family's other kernels walk: an
// atomic instruction's lanes then lie 16 bytes apart -- the variant DESIGN 4.18 measures this walk against (2.7 times slower on one
// hop of block motion).
//
// THE CLAMP (vp8_trace_read.hip.h) guards WRITES here: every trace value goes through trace_clamp before an address is formed from
// it, so a trace entry nobody wrote scatters garbage inside the job's two destination entries and never a byte outside them.
//
// vp8_cover_*_kernel is entry_tensor_body (vp8_trace_read.hip.h) with CoverPlanes: a COUNT entry as a tensor [planes][gh][gw], of
// the count c an output takes plane COUNT holding min(c, 255) and plane SEEN c != 0.  Counts are data there and never addresses.
#include "vp8_trace_read.hip.h"
#include "vp8hip.h"

// grid: x = the workgroups that share an entry (L.S), y = the jobs of the launch.  first, count: entry 0 of each pool, or null.
extern "C" __global__ void __launch_bounds__(256)
vp8_invert_fill_kernel(uint8_t *first, size_t first_stride, uint8_t *count, size_t count_stride, InvertLaunch L)
{
    const InvertJob J = L.j[blockIdx.y];
    const unsigned n = (unsigned)L.dw * (unsigned)L.dh, step = gridDim.x * 256u;        // (dwords of an entry: below 2^28)
#pragma unroll
    for (int o = 0; o < 2; o++) {
        uint8_t *pool = o ? count : first;
        if (!pool) continue;                             // (the same for every lane)
        const unsigned v = o ? 0u : 0xffffffffu;
        g_u32p D = (g_u32p)(pool + (o ? count_stride : first_stride) * (size_t)J.dst);
        unsigned done = 0;
        if (o ? L.count_vec : L.first_vec) {
            done = n & ~3u;
#pragma unroll 1
            for (unsigned q = blockIdx.x * 256u + threadIdx.x; q < n >> 2; q += step) ((GLOBAL_AS u32x4_t *)D)[q] = u32x4_t{v, v, v, v};
        }
#pragma unroll 1
        for (unsigned i = done + blockIdx.x * 256u + threadIdx.x; i < n; i += step) D[i] = v;
    }
}

template <bool FIRST, bool COUNT>
__device__ __forceinline__ void invert_body(const uint8_t *__restrict__ pool, size_t pool_stride, uint8_t *first, size_t first_stride, uint8_t *count,
                                            size_t count_stride, const InvertLaunch &L)
{
    const InvertJob J = L.j[blockIdx.y];
    const int dw = L.dw, dh = L.dh;
    int y0, y1;
    tensor_share(0, dh, L.S, (int)blockIdx.x, y0, y1);
    const GLOBAL_AS unsigned *src = (const GLOBAL_AS unsigned *)(pool + pool_stride * (size_t)J.trace);
    GLOBAL_AS unsigned *F = FIRST ? (GLOBAL_AS unsigned *)(first + first_stride * (size_t)J.dst) : nullptr;
    GLOBAL_AS unsigned *C = COUNT ? (GLOBAL_AS unsigned *)(count + count_stride * (size_t)J.dst) : nullptr;
#ifndef INVERT_LANE_QUADS
    const unsigned p0 = (unsigned)y0 * (unsigned)dw, p1 = (unsigned)y1 * (unsigned)dw;       // (pixels of an entry: below 2^28)
#pragma unroll 1
    for (unsigned base = p0 + (threadIdx.x >> 6) * 256u + (threadIdx.x & 63u); base < p1; base += 1024u) {
        unsigned T[4];
#pragma unroll
        for (int i = 0; i < 4; i++) T[i] = base + 64u * i < p1 ? src[base + 64u * i] : 0u;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const unsigned p = base + 64u * i;
            if (p >= p1) continue;
            const unsigned y = p / (unsigned)dw, x = p - y * (unsigned)dw;
            int ax, ay;
            trace_clamp(T[i], dw, dh, ax, ay);           // 0 <= ax < dw, 0 <= ay < dh: a dword of the destination entry
            const size_t a = (size_t)ay * dw + ax;
            if constexpr (FIRST) (void)__hip_atomic_fetch_min(F + a, y << 16 | x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if constexpr (COUNT) (void)__hip_atomic_fetch_add(C + a, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
#else
    const int nrows = y1 - y0;
#pragma unroll 1
    for (TensorWalk t((dw + 3) >> 2); t.row < nrows; t.next()) {
        const int y = y0 + t.row, x = t.col << 2;
        const GLOBAL_AS unsigned *row = src + (size_t)y * dw;
        u32x4_t T = {0, 0, 0, 0};
        if (L.vec) T = load4_dword_aligned(row + x);     // (dw % 4 == 0: the four are the row's)
        else {
#pragma unroll
            for (int i = 0; i < 4; i++)
                if (x + i < dw) T[i] = row[x + i];
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
            if (x + i >= dw) continue;
            int ax, ay;
            trace_clamp(T[i], dw, dh, ax, ay);           // 0 <= ax < dw, 0 <= ay < dh: a dword of the destination entry
            const size_t a = (size_t)ay * dw + ax;
            if constexpr (FIRST) (void)__hip_atomic_fetch_min(F + a, (unsigned)y << 16 | (unsigned)(x + i), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if constexpr (COUNT) (void)__hip_atomic_fetch_add(C + a, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
#endif
}

// grid: x = the workgroups that share a job's rows (L.S), y = the jobs of the launch.  pool, first, count: entry 0 of each pool
#define INVERT_KERNEL(NAME, FIRST, COUNT)                                                                                                 \
    extern "C" __global__ void __launch_bounds__(256)                                                                                     \
    NAME(const uint8_t *__restrict__ pool, size_t pool_stride, uint8_t *first, size_t first_stride, uint8_t *count, size_t count_stride,  \
         InvertLaunch L)                                                                                                                  \
    {                                                                                                                                     \
        invert_body<FIRST, COUNT>(pool, pool_stride, first, first_stride, count, count_stride, L);                                        \
    }
INVERT_KERNEL(vp8_invert_first_kernel, true, false)
INVERT_KERNEL(vp8_invert_count_kernel, false, true)
INVERT_KERNEL(vp8_invert_both_kernel, true, true)

// (CoverPlanes: vp8_trace_read.hip.h, beside entry_tensor_body)
ENTRY_KERNEL(vp8_cover_u8_kernel, TENSOR_U8, CoverPlanes)
ENTRY_KERNEL(vp8_cover_f16_kernel, TENSOR_F16, CoverPlanes)
ENTRY_KERNEL(vp8_cover_f32_kernel, TENSOR_F32, CoverPlanes)
