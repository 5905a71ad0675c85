// The gather along the trace (vp8hip_trace_gather_async, vp8hip_trace.hip; include/vp8hip.h has the definition): a tensor of the
// caller's -- what a network made of a key frame: feature maps, logits, a label map -- carried to a later frame by that frame's
// trace.  Output (y, x) takes display pixel (sy, sx) by the centre map, the trace dword there names a position of the anchor
// picture, and the output is the source tensor at the cell under that position (NEAREST: the element's bits) or the four cells around
// it weighted in 1/256 steps (BILINEAR: single precision).  Source and output are the caller's tensors; no frame buffer is read.
//
// One body over element size, layout and filter.  What an output needs of its trace dword -- the clamp, the divisions, the offset of
// its cell in a channel's plane and the weights -- is a GatherTap, made ONCE per output and used for every channel.
//
// PLANAR [C][h][w], shaped as vp8_anchor_*_kernel (vp8_trace_residual.hip): grid x = the workgroups that share a job's output rows,
// y = the job, z = a group of L.cgroup channels (the trace is read again per group: 4 bytes an output against the group's channels).
// A lane takes four neighbouring outputs, at the display size their four trace dwords as one 16-byte load, and then, GATHER_UNROLL_*
// channels at a time, issues every element load of those channels before it uses one; a channel's four results leave as one piece
// where the tensor allows, neighbouring lanes' pieces side by side.  Block motion is piecewise constant, so a wave's loads of one
// channel mostly fall in a run of one source row.
//
// CHANNELS_LAST [h][w][C] is a row gather: C * elem contiguous bytes per output.  A workgroup takes a run of GATHER_RUN outputs: one
// lane per output leaves its tap in LDS, and after a barrier the lanes walk (output, 16-byte piece) pairs, consecutive lanes on
// consecutive bytes of the destination, each piece read from the row its output gathers (BILINEAR: from the four rows).  Tensors that
// do not take whole pieces are walked as (output, element) pairs the same way.
//
// THE CLAMP (vp8_trace_read.hip.h).  A trace value becomes an address here: gather_cell takes every one through trace_clamp, and the
// maps below take a position inside the picture to a cell inside the source grid, so no read falls outside the job's source tensor.
// Single precision only; no doubles, no atomics; offsets in size_t (C * gh * gw passes 2^32).
#include "vp8_trace_read.hip.h"

#ifndef GATHER_UNROLL_NEAREST
#define GATHER_UNROLL_NEAREST 4    // PLANAR: channels whose loads are in flight together: 16 loads a lane ...
#endif
#ifndef GATHER_UNROLL_BILINEAR
#define GATHER_UNROLL_BILINEAR 2   // ... and 32 (-DGATHER_UNROLL_BILINEAR=1: the variant DESIGN 4.15's measurement compares it with)
#endif

// what an output takes of the source grid: the offset of cell (cy, cx) -- BILINEAR: (y0, x0) -- in elements of a plane, and for
// BILINEAR the steps to x1 and y1 (0 at the last column / row) and the four weights over 65536, exact as floats
template <int FILTER> struct GatherTap;
template <> struct GatherTap<GATHER_NEAREST> { int o; };
template <> struct GatherTap<GATHER_BILINEAR> { int o, dx, dy; float w[4]; };

// the four weights of (wx, wy), each 0..255, over 65536: corners (y0, x0), (y0, x1), (y1, x0), (y1, x1)
__device__ __forceinline__ void gather_weights(int wx, int wy, float (&w)[4])
{
    const float k = 1.0f / 65536.0f;
    w[0] = (float)((256 - wx) * (256 - wy)) * k;
    w[1] = (float)(wx * (256 - wy)) * k;
    w[2] = (float)((256 - wx) * wy) * k;
    w[3] = (float)(wx * wy) * k;
}

// clamp(((2a + 1) * s * 128) / d - 128, 0, (s - 1) * 256) for 0 <= a < d: the centre of pixel a of d in 1/256 cells of s, from the
// cells' centres.  The definition's 64-bit quotient from two 32-bit divisions: with n = (2a + 1) * s = q * d + r (n < 2^29, r < 2^14),
// (128 n) / d = 128 q + (128 r) / d.
__device__ __forceinline__ int gather_pos256(int a, int s, int d)
{
    const unsigned n = (unsigned)(2 * a + 1) * (unsigned)s;
    const unsigned q = n / (unsigned)d, r = n - q * (unsigned)d;
    const int p = (int)(q * 128u + (r * 128u) / (unsigned)d) - 128;
    return min(max(p, 0), (s - 1) * 256);
}

// trace dword -> the offset of its first cell, and for BILINEAR the steps dx (0 / 1) and dy (0 / sw) to the other three and wx, wy
template <int FILTER>
__device__ __forceinline__ int gather_cell(unsigned t, const GatherLaunch &L, int &dx, int &dy, int &wx, int &wy)
{
    int ax, ay;
    trace_clamp(t, L.g.dw, L.g.dh, ax, ay);
    if constexpr (FILTER == GATHER_NEAREST) {
        dx = dy = wx = wy = 0;
        return tensor_src(ay, L.g.dh, L.sh) * L.sw + tensor_src(ax, L.g.dw, L.sw);    // the cell under the pixel's centre
    } else {
        const int px = gather_pos256(ax, L.sw, L.g.dw), py = gather_pos256(ay, L.sh, L.g.dh);
        const int x0 = px >> 8, y0 = py >> 8;
        wx = px & 255; wy = py & 255;
        dx = x0 + 1 < L.sw;
        dy = y0 + 1 < L.sh ? L.sw : 0;
        return y0 * L.sw + x0;
    }
}

template <int FILTER>
__device__ __forceinline__ void gather_tap(unsigned t, const GatherLaunch &L, GatherTap<FILTER> &tap)
{
    int dx, dy, wx, wy;
    tap.o = gather_cell<FILTER>(t, L, dx, dy, wx, wy);
    if constexpr (FILTER == GATHER_BILINEAR) {
        tap.dx = dx; tap.dy = dy;
        gather_weights(wx, wy, tap.w);
    }
}

template <int ES> __device__ __forceinline__ float gather_float(unsigned bits)
{
    if constexpr (ES == 4) return __uint_as_float(bits);
    else return __half2float(__ushort_as_half((unsigned short)bits));
}

// the four corners' bits -> the result's: four weighted products summed in single precision, the half rounded once to nearest-even.
// All the weight on the first corner (the only one that can have it) gives that corner's bits: the sum would turn -0 into +0.
template <int ES>
__device__ __forceinline__ unsigned gather_blend(const float (&w)[4], unsigned a, unsigned b, unsigned c, unsigned d)
{
    float r = gather_float<ES>(a) * w[0];
    r = fmaf(gather_float<ES>(b), w[1], r);
    r = fmaf(gather_float<ES>(c), w[2], r);
    r = fmaf(gather_float<ES>(d), w[3], r);
    unsigned bits;
    if constexpr (ES == 4) bits = __float_as_uint(r);
    else bits = (unsigned)__half_as_ushort(__float2half_rn(r));
    return w[0] == 1.0f ? a : bits;
}

// UN channels from c of four neighbouring outputs: every load first, then the values, then the stores
template <int ES, int FILTER, int UN>
__device__ __forceinline__ void gather_planar_channels(const GLOBAL_AS typename TensorUint<ES>::T *sp, size_t splane, uint8_t *D, size_t gplane,
                                                       size_t pix, int c, const GatherTap<FILTER> (&tap)[4], int x, int gw, int vec)
{
    typedef typename TensorUint<ES>::T elem_t;
    constexpr int TAPS = FILTER == GATHER_NEAREST ? 1 : 4;
    unsigned v[UN][4][TAPS];
#pragma unroll
    for (int u = 0; u < UN; u++) {
        const GLOBAL_AS elem_t *pl = sp + (size_t)(c + u) * splane;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            v[u][i][0] = pl[tap[i].o];
            if constexpr (FILTER == GATHER_BILINEAR) {
                v[u][i][1] = pl[tap[i].o + tap[i].dx];
                v[u][i][2] = pl[tap[i].o + tap[i].dy];
                v[u][i][3] = pl[tap[i].o + tap[i].dy + tap[i].dx];
            }
        }
    }
#pragma unroll
    for (int u = 0; u < UN; u++) {
        unsigned e[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            if constexpr (FILTER == GATHER_NEAREST) e[i] = v[u][i][0];
            else e[i] = gather_blend<ES>(tap[i].w, v[u][i][0], v[u][i][1], v[u][i][2], v[u][i][3]);
        }
        uint8_t *o = D + ((size_t)(c + u) * gplane + pix) * ES;
        if (vec) tensor_store4<ES>(o, e);
        else {
#pragma unroll
            for (int i = 0; i < 4; i++)
                if (x + i < gw) ((GLOBAL_AS elem_t *)o)[i] = (elem_t)e[i];
        }
    }
}

template <int ES, int FILTER>
__device__ __forceinline__ void gather_planar(const uint8_t *__restrict__ pool, size_t pool_stride, const uint8_t *__restrict__ src, size_t src_stride,
                                              uint8_t *__restrict__ dst, size_t dst_stride, const GatherLaunch &L)
{
    typedef typename TensorUint<ES>::T elem_t;
    constexpr int UN = FILTER == GATHER_NEAREST ? GATHER_UNROLL_NEAREST : GATHER_UNROLL_BILINEAR;
    const int f = (int)blockIdx.y;
    const GatherJob J = L.j[f];
    const int gw = L.g.gw, gh = L.g.gh;
    int y0, y1;
    tensor_share(0, gh, L.g.S, (int)blockIdx.x, y0, y1);
    const int c0 = (int)blockIdx.z * L.cgroup, c1 = min(L.C, c0 + L.cgroup);
    const uint8_t *trace = pool + pool_stride * (size_t)J.trace;
    const GLOBAL_AS elem_t *sp = (const GLOBAL_AS elem_t *)(src + src_stride * (size_t)J.src);
    uint8_t *D = dst + dst_stride * (size_t)f;
    const size_t splane = (size_t)L.sh * L.sw, gplane = (size_t)gh * gw;
    const int nrows = y1 - y0;
#pragma unroll 1
    for (TensorWalk t((gw + 3) >> 2); t.row < nrows; t.next()) {
        const int y = y0 + t.row, x = t.col << 2;
        const TraceQuad q = trace_read4(trace, L.g, y, x);
        GatherTap<FILTER> tap[4];
#pragma unroll
        for (int i = 0; i < 4; i++) gather_tap<FILTER>(q.T[i], L, tap[i]);
        const size_t pix = (size_t)y * gw + x;
        int c = c0;
#pragma unroll 1
        for (; c + UN <= c1; c += UN) gather_planar_channels<ES, FILTER, UN>(sp, splane, D, gplane, pix, c, tap, x, gw, L.g.vec);
#pragma unroll 1
        for (; c < c1; c++) gather_planar_channels<ES, FILTER, 1>(sp, splane, D, gplane, pix, c, tap, x, gw, L.g.vec);
    }
}

// a 16-byte piece of the four rows of an output -> the piece of its result: 16 / ES elements
template <int ES>
__device__ __forceinline__ u32x4_t gather_blend_piece(const float (&w)[4], u32x4_t a, u32x4_t b, u32x4_t c, u32x4_t d)
{
    u32x4_t r;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if constexpr (ES == 4) r[k] = gather_blend<4>(w, a[k], b[k], c[k], d[k]);
        else r[k] = gather_blend<2>(w, a[k] & 0xffffu, b[k] & 0xffffu, c[k] & 0xffffu, d[k] & 0xffffu) |
                    gather_blend<2>(w, a[k] >> 16, b[k] >> 16, c[k] >> 16, d[k] >> 16) << 16;
    }
    return r;
}

// the tap an output left in LDS: the offset of its first cell; BILINEAR: wx | wy << 8 | a column to the right << 16 | a row below << 17
template <int FILTER>
__device__ __forceinline__ void gather_lds_tap(const unsigned *s_o, const unsigned *s_w, int k, int sw, size_t (&cell)[4], float (&w)[4])
{
    cell[0] = s_o[k];
    if constexpr (FILTER == GATHER_BILINEAR) {
        const unsigned p = s_w[k];
        const int wx = (int)(p & 255u), wy = (int)((p >> 8) & 255u);
        const size_t dx = (p >> 16) & 1u, dy = (p >> 17) & 1u ? (size_t)sw : 0;
        cell[1] = cell[0] + dx; cell[2] = cell[0] + dy; cell[3] = cell[0] + dy + dx;
        gather_weights(wx, wy, w);
    }
}

template <int ES, int FILTER>
__device__ __forceinline__ void gather_rows(const uint8_t *__restrict__ pool, size_t pool_stride, const uint8_t *__restrict__ src, size_t src_stride,
                                            uint8_t *__restrict__ dst, size_t dst_stride, const GatherLaunch &L)
{
    typedef typename TensorUint<ES>::T elem_t;
    __shared__ unsigned s_o[GATHER_RUN];
    __shared__ unsigned s_w[FILTER == GATHER_BILINEAR ? GATHER_RUN : 1];
    const int f = (int)blockIdx.y;
    const GatherJob J = L.j[f];
    const int gw = L.g.gw, total = L.g.gh * gw;              // (below 2^28)
    const int first = (int)blockIdx.x * GATHER_RUN, tid = (int)threadIdx.x;
    const int nout = min(GATHER_RUN, total - first);
    if (tid < nout) {
        const int o = first + tid, y = o / gw, x = o - y * gw;
        const int sy = tensor_src(y, L.g.gh, L.g.dh), sx = trace_col(L.g, x);
        const unsigned t = ((const GLOBAL_AS unsigned *)(pool + pool_stride * (size_t)J.trace))[(size_t)sy * L.g.dw + sx];
        int dx, dy, wx, wy;
        s_o[tid] = (unsigned)gather_cell<FILTER>(t, L, dx, dy, wx, wy);
        if constexpr (FILTER == GATHER_BILINEAR) s_w[tid] = (unsigned)wx | (unsigned)wy << 8 | (unsigned)dx << 16 | (dy ? 1u << 17 : 0u);
    }
    __syncthreads();
    const size_t rowb = (size_t)L.C * ES;                    // an output's bytes, a cell's bytes
    const uint8_t *S = src + src_stride * (size_t)J.src;
    uint8_t *D = dst + dst_stride * (size_t)f + (size_t)first * rowb;
    if (L.g.vec) {
        // (output, 16-byte piece): UN pairs a lane in flight
        constexpr int UN = FILTER == GATHER_NEAREST ? 4 : 2;
        constexpr int TAPS = FILTER == GATHER_NEAREST ? 1 : 4;
        const int P = (int)(rowb >> 4);
        TensorWalk t(P);
#pragma unroll 1
        while (t.row < nout) {
            u32x4_t v[UN][TAPS];
            float w[UN][4];
            size_t to[UN];
            bool on[UN];
#pragma unroll
            for (int u = 0; u < UN; u++) {
                on[u] = t.row < nout;
                if (on[u]) {
                    size_t cell[4];
                    gather_lds_tap<FILTER>(s_o, s_w, t.row, L.sw, cell, w[u]);
                    const size_t in_row = (size_t)t.col << 4;
                    to[u] = (size_t)t.row * rowb + in_row;
#pragma unroll
                    for (int k = 0; k < TAPS; k++) v[u][k] = *(const GLOBAL_AS u32x4_t *)(S + cell[k] * rowb + in_row);
                }
                t.next();
            }
#pragma unroll
            for (int u = 0; u < UN; u++) {
                if (!on[u]) continue;
                if constexpr (FILTER == GATHER_NEAREST) *(GLOBAL_AS u32x4_t *)(D + to[u]) = v[u][0];
                else *(GLOBAL_AS u32x4_t *)(D + to[u]) = gather_blend_piece<ES>(w[u], v[u][0], v[u][1], v[u][2], v[u][3]);
            }
        }
    } else {
        // (output, element), each element once
#pragma unroll 1
        for (TensorWalk t(L.C); t.row < nout; t.next()) {
            size_t cell[4];
            float w[4];
            gather_lds_tap<FILTER>(s_o, s_w, t.row, L.sw, cell, w);
            const GLOBAL_AS elem_t *sp = (const GLOBAL_AS elem_t *)S + t.col;
            unsigned e;
            if constexpr (FILTER == GATHER_NEAREST) e = sp[cell[0] * L.C];
            else e = gather_blend<ES>(w, sp[cell[0] * L.C], sp[cell[1] * L.C], sp[cell[2] * L.C], sp[cell[3] * L.C]);
            ((GLOBAL_AS elem_t *)D)[(size_t)t.row * L.C + t.col] = (elem_t)e;
        }
    }
}

// PLANAR: grid x = the workgroups that share a job's output rows (L.g.S), y = the jobs of the launch, z = the groups of channels.
// CHANNELS_LAST: grid x = the runs of GATHER_RUN outputs, y = the jobs.  pool: entry 0; src: source tensor 0; dst: the launch's first output.
#define GATHER_KERNEL(NAME, ES, LAYOUT, FILTER)                                                                                           \
    extern "C" __global__ void __launch_bounds__(256)                                                                                     \
    NAME(const uint8_t *__restrict__ pool, size_t pool_stride, const uint8_t *__restrict__ src, size_t src_stride,                        \
         uint8_t *__restrict__ dst, size_t dst_stride, GatherLaunch L)                                                                    \
    {                                                                                                                                     \
        if constexpr (LAYOUT == GATHER_PLANAR) gather_planar<ES, FILTER>(pool, pool_stride, src, src_stride, dst, dst_stride, L);         \
        else gather_rows<ES, FILTER>(pool, pool_stride, src, src_stride, dst, dst_stride, L);                                             \
    }
GATHER_KERNEL(vp8_gather_planar_nearest_1_kernel, 1, GATHER_PLANAR, GATHER_NEAREST)
GATHER_KERNEL(vp8_gather_planar_nearest_2_kernel, 2, GATHER_PLANAR, GATHER_NEAREST)
GATHER_KERNEL(vp8_gather_planar_nearest_4_kernel, 4, GATHER_PLANAR, GATHER_NEAREST)
GATHER_KERNEL(vp8_gather_rows_nearest_1_kernel, 1, GATHER_CHANNELS_LAST, GATHER_NEAREST)
GATHER_KERNEL(vp8_gather_rows_nearest_2_kernel, 2, GATHER_CHANNELS_LAST, GATHER_NEAREST)
GATHER_KERNEL(vp8_gather_rows_nearest_4_kernel, 4, GATHER_CHANNELS_LAST, GATHER_NEAREST)
GATHER_KERNEL(vp8_gather_planar_bilinear_2_kernel, 2, GATHER_PLANAR, GATHER_BILINEAR)
GATHER_KERNEL(vp8_gather_planar_bilinear_4_kernel, 4, GATHER_PLANAR, GATHER_BILINEAR)
GATHER_KERNEL(vp8_gather_rows_bilinear_2_kernel, 2, GATHER_CHANNELS_LAST, GATHER_BILINEAR)
GATHER_KERNEL(vp8_gather_rows_bilinear_4_kernel, 4, GATHER_CHANNELS_LAST, GATHER_BILINEAR)
