// Reading a trace (include/vp8hip.h: one dword per pixel of the display-size grid, x' in the low int16 and y' in the high one), once
// for the kernels that do: vp8_trace_kernel for a reference's trace, and the readers of a pool entry laid under an output grid
// (TraceGrid, vp8_common.hip.h) -- vp8_flow_*_kernel (vp8_trace.hip), vp8_anchor_*_kernel (vp8_trace_residual.hip) and
// vp8_gather_*_kernel (vp8_trace_gather.hip); and vp8_trace_wear.hip, whose pool has a trace pool's geometry and whose dwords are
// counters: vp8_wear_kernel gathers a reference's as vp8_trace_kernel does, vp8_wear_*_kernel reads an entry through trace_read4;
// and vp8_trace_invert.hip: vp8_invert_*_kernel scatters a trace onto the anchor's grid, vp8_cover_*_kernel reads an entry of its
// COUNT pool -- a trace pool's geometry again, the dwords counts -- through trace_read4.
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
