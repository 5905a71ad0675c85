// Accumulated motion (vp8hip_frames_trace_async and vp8hip_trace_flow_async, vp8hip_trace.hip; include/vp8hip.h has the
// definitions).  The TRACE of a frame says, for every pixel of the display-size luma grid, which position of the anchor picture --
// the key frame that started the group -- it descends from: one dword per pixel, x' in the low int16 and y' in the high one.  An
// inter frame's trace is one hop: the pixel's vector, rounded to whole pixels and clamped to the picture, points into the reference
// its macroblock was predicted from, and the pixel takes the dword that reference's trace holds there.  Traces live in a pool in
// the caller's device memory; the references are entries of it.
//
// vp8_trace_kernel is trace_hop_body (vp8_trace_read.hip.h has the walk) with TraceHop: the LDS dword of a macroblock is its record's
// first (y_mode, ref_frame), a key frame writes the identity, and a pixel takes the gathered dword as it is.
//
// vp8_flow_*_kernel is entry_tensor_body (vp8_trace_read.hip.h) with FlowPlanes: a pool entry as a tensor [2][gh][gw], output (y, x)
// holding T.x - sx, T.y - sy of the trace pixel (sy, sx) it takes; both planes always.
// Integer and conversion arithmetic only; trace values are data and never become addresses.
#include "vp8_trace_read.hip.h"
#include "vp8hip.h"

struct TraceHop {
    static __device__ __forceinline__ unsigned stage(const GLOBAL_AS unsigned *rec) { return rec[0]; }
    static __device__ __forceinline__ unsigned ref(unsigned d) { return (d >> 16) & 255u; }
    static __device__ __forceinline__ unsigned key(int x, int y, int i) { return ((unsigned)x | (unsigned)y << 16) + i; }
    static __device__ __forceinline__ unsigned inc(unsigned, int, bool) { return 0; }
    static __device__ __forceinline__ unsigned take(unsigned g, unsigned, bool) { return g; }
};

// grid: x = the groups of macroblock rows of a frame, y = the jobs of the launch.  slot_base: IR slot 0, slot_bytes apart, records
// at o_mbx and vectors at o_mvs inside; pool: entry 0, pool_stride apart.
extern "C" __global__ void __launch_bounds__(256)
vp8_trace_kernel(const char *__restrict__ slot_base, size_t slot_bytes, size_t o_mbx, size_t o_mvs, uint8_t *pool, size_t pool_stride, TraceLaunch L)
{
    trace_hop_body<TraceHop>(slot_base, slot_bytes, o_mbx, o_mvs, pool, pool_stride, L);
}

struct FlowPlanes {
    static constexpr int N = 2;
    static constexpr bool MASKED = false;
    static __device__ __forceinline__ int value(const TraceQuad &q, int i, int c) { return c == 0 ? trace_x(q.T[i]) - q.sx[i] : trace_y(q.T[i]) - q.sy; }
};
ENTRY_KERNEL(vp8_flow_i16_kernel, TENSOR_I16, FlowPlanes)
ENTRY_KERNEL(vp8_flow_f16_kernel, TENSOR_F16, FlowPlanes)
ENTRY_KERNEL(vp8_flow_f32_kernel, TENSOR_F32, FlowPlanes)
