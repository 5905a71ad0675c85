// Reading a trace (include/vp8hip.h: one dword per pixel of the display-size grid, x' in the low int16 and y' in the high one), once
// for the kernels that do, and for those whose pool has a trace pool's geometry and other dwords (vp8_trace_wear.hip: counters;
// vp8_trace_invert.hip's COUNT pool: counts).  Three things live here:
// - the pieces of a reader of a pool entry laid under an output grid (TraceGrid, vp8_common.hip.h), down to trace_read4: what
//   vp8_anchor_*_kernel (vp8_trace_residual.hip), vp8_gather_*_kernel (vp8_trace_gather.hip) and entry_tensor_body are made of, and
//   the scatter of vp8_invert_*_kernel takes its clamp from;
// - trace_hop_body, the hop along the slots' vectors that makes an entry of its references: vp8_trace_kernel and vp8_wear_kernel;
// - entry_tensor_body, a pool entry as a tensor: vp8_flow_*_kernel (vp8_trace.hip), vp8_wear_*_kernel and vp8_cover_*_kernel.
//
// THE CLAMP.  In vp8_trace.hip a trace value is data; in the other two files it becomes an address.  There every value goes through
// trace_clamp before anything is formed from it, so a pool entry nobody wrote yields garbage values and never a read outside the
// picture; what lies behind the picture -- the anchor's frame buffer, the job's source tensor -- is the caller's to reach from a
// position inside it.  trace_clamp is the one place that makes a position of a trace dword: a reader does not unpack one by itself.
// vp8_trace_invert.hip is a fourth file where a trace value becomes an address (vp8_trace_wear.hip is none: its positions come from
// the slot's vectors), and the first where that address is WRITTEN: vp8_invert_*_kernel does an atomic on dword ay * dw + ax of the
// job's destination entries.  The rule is the same and now guards writes -- the position comes out of trace_clamp, 0 <= ax < dw and
// 0 <= ay < dh, and nothing else of the dword takes part in the address --, so a trace entry nobody wrote scatters garbage inside
// the destination entries, d_w * d_h dwords each, and never a byte outside them.
#pragma once
#include "vp8_tensor_out.hip.h"

// Four neighbouring dwords at a dword-aligned address: one global_load_dwordx4 (gfx950 under HSA takes it at any dword; the
// compiler emits it for a vector type of alignment 4), or with -DTRACE_GATHER_DWORDS four global_load_dword -- the variant
// DESIGN 4.13's measurement compares it with.
#ifdef TRACE_GATHER_DWORDS
__device__ __forceinline__ u32x4_t load4_dword_aligned(const GLOBAL_AS unsigned *p)
{
    const volatile GLOBAL_AS unsigned *q = p;
    return u32x4_t{q[0], q[1], q[2], q[3]};
}
#else
typedef u32x4_t u32x4_dword_t __attribute__((aligned(4)));
__device__ __forceinline__ u32x4_t load4_dword_aligned(const GLOBAL_AS unsigned *p) { return *(const GLOBAL_AS u32x4_dword_t *)p; }
#endif

// the position a trace dword holds as written, and clamped to the picture dw x dh
__device__ __forceinline__ int trace_x(unsigned t) { return (int)(short)(t & 0xffffu); }
__device__ __forceinline__ int trace_y(unsigned t) { return (int)t >> 16; }
__device__ __forceinline__ void trace_clamp(unsigned t, int dw, int dh, int &ax, int &ay)
{
    ax = min(max(trace_x(t), 0), dw - 1);
    ay = min(max(trace_y(t), 0), dh - 1);
}

// the column output x reads; and whether outputs x .. x + 3 read columns x .. x + 3: at the display size, for a group inside the row
__device__ __forceinline__ int trace_col(const TraceGrid &G, int x) { return G.xmode == SIDE_X_DISPLAY ? x : tensor_src(x, G.gw, G.dw); }
__device__ __forceinline__ bool trace_whole(const TraceGrid &G, int x) { return G.xmode == SIDE_X_DISPLAY && x + 3 < G.gw; }

// The dwords T of outputs x .. x + 3 of row y (x a multiple of 4; those past the row repeat its last) in pool entry `entry`, and the
// row sy and the columns sx they were read at: one load where trace_whole, else four.  Values, not arrays by reference: through
// references the compiler merges the two paths' stores, and the arrays stay in scratch.  vp8_anchor_*_kernel, which reads the frame
// between these loads, and the row gather, a lane an output, are written with the pieces above (what this cost them).
typedef int i32x4_t __attribute__((ext_vector_type(4)));
struct TraceQuad { u32x4_t T; i32x4_t sx; int sy; };
__device__ __forceinline__ TraceQuad trace_read4(const uint8_t *entry, const TraceGrid &G, int y, int x)
{
    TraceQuad q;
    q.sy = tensor_src(y, G.gh, G.dh);
    const GLOBAL_AS unsigned *row = (const GLOBAL_AS unsigned *)entry + (size_t)q.sy * G.dw;
    if (trace_whole(G, x)) {
        q.T = load4_dword_aligned(row + x);
        q.sx = i32x4_t{x, x + 1, x + 2, x + 3};
    } else {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            q.sx[i] = trace_col(G, min(x + i, G.gw - 1));
            q.T[i] = row[q.sx[i]];
        }
    }
    return q;
}

// ONE HOP of a pool whose entries chain through the slots' records and vectors: what vp8_trace_kernel (vp8_trace.hip) and
// vp8_wear_kernel (vp8_trace_wear.hip) are.  Small input, large output, as vp8_side.hip: a workgroup takes a group of R macroblock rows
// and the display rows inside them.  It stages what a hop reads of the slot into LDS -- one dword a macroblock, made of its record by
// Hop::stage, and the rows' vectors, those with 16-byte loads: 68 bytes a macroblock -- and then a lane makes four neighbouring pixels:
// one 4x4 block's row, so one vector, one reference and, where the clamp does not bite, sixteen contiguous bytes of the reference's
// entry, aligned to a dword only.  A key frame writes Hop::key and reads nothing.  Stores as in vp8_side.hip: whole 16-byte pieces
// where the pool allows, else element by element.  Job, references and the key-frame bit travel in the kernel arguments.
// Hop says what the pool's dwords are:
//   stage(rec)    the LDS dword of the macroblock whose record (vp8ir_mb, 32 dwords) is at rec
//   ref(d)        the reference frame that dword holds
//   key(x, y, i)  what a key frame writes at pixel (x + i, y)
//   inc(d, k, row_edge)   what a hop adds for the four pixels of a lane: d their macroblock's LDS dword, k their 4x4 block, and
//                 whether the clamp moved the row they gather at
//   take(g, inc, col_edge)   what a pixel takes of the dword g gathered from its reference, and whether the clamp moved its column
// The positions come from the slot's vectors, clamped to the picture; no address is formed from a pool value.
template <class Hop>
__device__ __forceinline__ void trace_hop_body(const char *__restrict__ slot_base, size_t slot_bytes, size_t o_mbx, size_t o_mvs, uint8_t *pool,
                                               size_t pool_stride, const TraceLaunch &L)
{
    extern __shared__ __attribute__((aligned(16))) unsigned trace_lds[];
    const TraceJob J = L.j[blockIdx.y];
    const int dw = L.dw, dh = L.dh, cols = L.mb_cols;
    const int m0 = (int)blockIdx.x * L.R, m1 = min(m0 + L.R, L.mb_rows);
    const int y0 = 16 * m0, y1 = min(16 * m1, dh);
    const bool key = J.key != 0;
    const unsigned *lrec = trace_lds + (size_t)L.R * cols * 16, *lmvs = trace_lds;        // vectors first: 16-byte pieces
    if (!key) {
        const char *slot = slot_base + slot_bytes * (size_t)J.slot;
        const GLOBAL_AS unsigned *grec = (const GLOBAL_AS unsigned *)(slot + o_mbx) + (size_t)m0 * cols * 32;
        const GLOBAL_AS u32x4_t *gmvs = (const GLOBAL_AS u32x4_t *)(slot + o_mvs) + (size_t)m0 * cols * 4;
        const int nmb = (m1 - m0) * cols;
#pragma unroll 1
        for (int t = threadIdx.x; t < nmb; t += 256) trace_lds[(size_t)L.R * cols * 16 + t] = Hop::stage(grec + t * 32);
#pragma unroll 1
        for (int t = threadIdx.x; t < nmb * 4; t += 256) ((u32x4_t *)trace_lds)[t] = gmvs[t];
        __syncthreads();
    }

    uint8_t *D = pool + pool_stride * (size_t)J.dst;
    const int nrows = y1 - y0;
#pragma unroll 1
    for (TensorWalk t((dw + 3) >> 2); t.row < nrows; t.next()) {
        const int y = y0 + t.row, x = t.col << 2;
        unsigned e[4] = {Hop::key(x, y, 0), Hop::key(x, y, 1), Hop::key(x, y, 2), Hop::key(x, y, 3)};
        if (!key) {
            const int mb = ((y >> 4) - m0) * cols + (x >> 4);
            const unsigned rec = lrec[mb], ref = Hop::ref(rec);
            // an intra macroblock is held in place through the last frame
            const int pi = ref <= VP8IR_LAST_FRAME ? J.ref[0] : ref == VP8IR_GOLDEN_FRAME ? J.ref[1] : ref == VP8IR_ALTREF_FRAME ? J.ref[2] : -1;
            if (pi >= 0) {
                const int k = ((y >> 2) & 3) * 4 + ((x >> 2) & 3);
                const unsigned v = ref == VP8IR_INTRA_FRAME ? 0u : lmvs[mb * 16 + k];
                const int dx = (((int)v >> 16) + 4) >> 3, dy = ((int)(short)(v & 0xffffu) + 4) >> 3;       // col in the high half
                const int uy = y + dy, sy = min(max(uy, 0), dh - 1), sx = x + dx;
                const unsigned inc = Hop::inc(rec, k, sy != uy);
                const GLOBAL_AS unsigned *row = (const GLOBAL_AS unsigned *)(pool + pool_stride * (size_t)pi) + (size_t)sy * dw;
                if (sx >= 0 && sx + 3 < dw) {
                    const u32x4_t g = load4_dword_aligned(row + sx);
#pragma unroll
                    for (int i = 0; i < 4; i++) e[i] = Hop::take(g[i], inc, false);
                } else {
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const int cx = min(max(sx + i, 0), dw - 1);
                        e[i] = Hop::take(row[cx], inc, cx != sx + i);
                    }
                }
            }
        }
        uint8_t *o = D + ((size_t)y * dw + x) * 4;
        if (L.vec) tensor_store4<4>(o, e);
        else {
#pragma unroll
            for (int i = 0; i < 4; i++)
                if (x + i < dw) ((g_u32p)o)[i] = e[i];
        }
    }
}

// A POOL ENTRY AS A TENSOR [planes][gh][gw]: what vp8_flow_*_kernel (vp8_trace.hip), vp8_wear_*_kernel (vp8_trace_wear.hip) and
// vp8_cover_*_kernel (vp8_trace_invert.hip) are.  Output (y, x) takes the entry's dword at (sy, sx) by the centre map, read through
// trace_read4, and each plane holds an int made of it, converted as the side tensors are: four at a time by tensor_values4, stored
// as one piece where the tensor allows, else element by element.  Planes says what the planes are:
//   N                the planes there are
//   MASKED           whether EntryLaunch::planes picks among them (plane c where bit c is set, in bit order) or all are made
//   value(q, i, c)   plane c's int for output i of the four read as q
// The entry's dwords are data and never become addresses.
template <int DTYPE, class Planes>
__device__ __forceinline__ void entry_tensor_body(const uint8_t *__restrict__ pool, size_t pool_stride, uint8_t *__restrict__ dst, size_t dst_stride,
                                                  const EntryLaunch &L)
{
    typedef typename TensorElem<DTYPE>::T elem_t;
    constexpr int ES = (int)sizeof(elem_t);
    const int f = (int)blockIdx.y;
    const int gw = L.g.gw, gh = L.g.gh;
    int y0, y1;
    tensor_share(0, gh, L.g.S, (int)blockIdx.x, y0, y1);
    const uint8_t *src = pool + pool_stride * (size_t)L.idx[f];
    uint8_t *D = dst + dst_stride * f;
    const size_t plane = (size_t)gh * gw;
    const int nrows = y1 - y0;
#pragma unroll 1
    for (TensorWalk t((gw + 3) >> 2); t.row < nrows; t.next()) {
        const int y = y0 + t.row, x = t.col << 2;
        const TraceQuad q = trace_read4(src, L.g, y, x);
        uint8_t *o = D + ((size_t)y * gw + x) * ES;
#pragma unroll
        for (int c = 0; c < Planes::N; c++) {
            if (Planes::MASKED && !(L.planes >> c & 1u)) continue;       // (the same for every lane)
            int v[4];
#pragma unroll
            for (int i = 0; i < 4; i++) v[i] = Planes::value(q, i, c);
            unsigned e[4];
            tensor_values4<DTYPE>(v, L.scale[c], e);
            if (L.g.vec) tensor_store4<ES>(o, e);
            else {
#pragma unroll
                for (int i = 0; i < 4; i++)
                    if (x + i < gw) ((GLOBAL_AS elem_t *)o)[i] = (elem_t)e[i];
            }
            o += plane * ES;
        }
    }
}

// grid: x = the workgroups that share a frame's output rows (L.g.S), y = the frames of the launch.  pool: entry 0; dst: the launch's
// first frame.
#define ENTRY_KERNEL(NAME, DTYPE, PLANES)                                                                                                 \
    extern "C" __global__ void __launch_bounds__(256)                                                                                     \
    NAME(const uint8_t *__restrict__ pool, size_t pool_stride, uint8_t *__restrict__ dst, size_t dst_stride, EntryLaunch L)               \
    {                                                                                                                                     \
        entry_tensor_body<DTYPE, PLANES>(pool, pool_stride, dst, dst_stride, L);                                                          \
    }

// What the dwords of the two pools that are handed out plane by plane hold, for entry_tensor_body and for the histograms of the same
// tensors (vp8_hist.hip).  A wear dword (vp8_trace_wear.hip): four byte counters, HOPS, INTRA, EDGE, CODED from the low byte up.
struct WearPlanes {
    static constexpr int N = 4;
    static constexpr bool MASKED = true;
    static __device__ __forceinline__ int value(const TraceQuad &q, int i, int c) { return (int)(q.T[i] >> 8 * c & 255u); }
};
// A COUNT dword (vp8_trace_invert.hip): plane COUNT holds min(c, 255), plane SEEN c != 0.
struct CoverPlanes {
    static constexpr int N = 2;
    static constexpr bool MASKED = true;
    static __device__ __forceinline__ int value(const TraceQuad &q, int i, int c) { return c == 0 ? (int)min(q.T[i], 255u) : (int)(q.T[i] != 0u); }
};
