// Block motion search between pictures (vp8hip_frames_motion_async; vp8hip_motion.hip has the plan, include/vp8hip.h the definition):
// per macroblock of frame buffer fb the whole-pixel displacement into ref_fb that vp8_full_search_sad_c finds -- every candidate of
// the square of side 2d around a centre, valued by vp8_sad16x16_c plus mvsad_err_cost, the first strictly smallest kept -- and what
// that match costs.  A workgroup owns one macroblock of one job; nothing but its outputs is written.
//
// WINDOW.  The candidates read rows cy - d .. cy + d + 14 and columns cx - d .. cx + d + 14 of the reference picture around the
// macroblock.  The workgroup stages them in LDS once, through frame_edge4 (vp8_frame_read.hip.h: the coded area extended by
// coordinate clamps, from either form of the frame buffer), with byte 0 of a window row the column cx - d: a staged dword is
// one aligned dword of the picture where cx - d is a multiple of 4 (always, without a centre tensor and with d a multiple of 4),
// else two shifted together.  All clamps are spent here; the loop below has none.  The block's 64 dwords and the cost table go
// to LDS beside it.
// ITEMS.  A lane takes an item: MOTION_ROWS candidate rows by four neighbouring candidate columns.  It walks the 15 + MOTION_ROWS
// window rows the item touches, reads five dwords of each (4-aligned: ds_read2_b32 and ds_read_b32) and issues, per candidate row
// the window row serves and per block dword, one v_qsad_pk_u16_u8: eight window bytes against four block bytes, four sliding
// sums onto a packed accumulator (255 * 256 < 2^16: no carry between the four).  Four block rows are in registers at a time.  Lanes of
// a wave lie on neighbouring items of a row of items; the plan pads the row pitch so that the item rows a half-wave spans fall
// on different banks.
// KEYS.  A candidate's key is value << 32 | position in the reference's order: 0 for the centre, 1 + row * 2d + column for the
// loop.  Candidates the reference's loop does not visit -- outside the UMV bounds, or in the padding of the last item -- get the
// key "never", by a select, not a branch.  The smallest key is the reference's answer: strict < in its order.  A lane takes the
// minimum of its keys, the wave of its lanes' (ds_bpermute), the workgroup of its waves' in LDS: a minimum of distinct 64-bit
// numbers, the same bits whatever order lanes and waves arrive in.
// SECOND PASS.  The first wave takes a dword of the block per lane and the winner's bytes from the window in LDS, and makes the
// sums of SSE, VAR, SAD0 and SRCVAR with v_dot4_u32_u8 / v_sad_u8, only for the planes asked for; lane 0 stores.
#include "vp8_frame_read.hip.h"
#include "vp8hip.h"

typedef unsigned long long motion_key_t;
static_assert(MOTION_ROWS == 4, "the item loop names its four accumulators");
#define MOTION_NEVER (~0ull)
#define MOTION_COST_ROW (2 * MOTION_MAX_D + 2)
#define MOTION_LDS_KEYS 0                                    // dword offsets of the pieces of a workgroup's LDS: 4 keys,
#define MOTION_LDS_BLOCK 8                                   // the block's 64 dwords (16-byte aligned),
#define MOTION_LDS_COST (MOTION_LDS_BLOCK + 64)              // the cost table, a dword per entry,
#define MOTION_LDS_WINDOW (MOTION_LDS_COST + 2 * MOTION_COST_ROW)    // the window (vp8hip_motion.hip sizes the launch by this)

// a wave's smallest key in its lane 0
__device__ __forceinline__ motion_key_t motion_wave_min(motion_key_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const motion_key_t w = __shfl_down(v, o, 64);
        v = w < v ? w : v;
    }
    return v;
}

// a wave's sum in its lane 0
__device__ __forceinline__ unsigned motion_wave_sum(unsigned v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// the window whose first byte is E(y0, x0) into LDS, from the form FORM of R.  The loads of an unrolled round are all in flight
// before the first is waited for: nothing between them branches
template <int FORM>
__device__ __forceinline__ void motion_stage(unsigned *win, const HistFrame &R, const MotionLaunch &L, int x0, int y0)
{
    const int pitch = L.pitch, step = (int)blockDim.x, adv_rows = step / pitch, adv_cols = step - adv_rows * pitch;
    const unsigned sh = (unsigned)x0 & 3u;        // (the same for every lane)
    // (row, col) of dword threadIdx.x + k * blockDim.x of the window, carried from one round to the next: one division, not one a round
    int row = (int)threadIdx.x / pitch, col = (int)threadIdx.x - row * pitch;
    if (!sh) {
#pragma unroll 4
        while (row < L.rows) {
            win[row * pitch + col] = frame_edge4<FORM>(R, L, x0 + 4 * col, y0 + row);
            col += adv_cols;
            row += adv_rows;
            if (col >= pitch) { col -= pitch; row++; }
        }
    } else {
        const int xa = x0 & ~3;
#pragma unroll 4
        while (row < L.rows) {
            win[row * pitch + col] = __builtin_amdgcn_alignbyte(frame_edge4<FORM>(R, L, xa + 4 * col + 4, y0 + row),
                                                                frame_edge4<FORM>(R, L, xa + 4 * col, y0 + row), sh);
            col += adv_cols;
            row += adv_rows;
            if (col >= pitch) { col -= pitch; row++; }
        }
    }
}

// grid: x = the macroblocks in raster order, y = the jobs of the launch; 64 to 256 threads; dynamic LDS: MOTION_LDS_WINDOW +
// L.rows * L.pitch dwords.  raster / tiles: frame buffer 0 in its two forms (vp8_scale_kernel's); centre / mv / stats: the launch's
// first tensors (null where L says there is none)
extern "C" __global__ void __launch_bounds__(256)
vp8_motion_frames_kernel(const uint8_t *__restrict__ raster, size_t fb_stride, const uint8_t *__restrict__ tiles, size_t tile_frame,
                         const uint8_t *__restrict__ centre, size_t centre_stride, uint8_t *__restrict__ mv, size_t mv_stride,
                         uint8_t *__restrict__ stats, size_t stats_stride, MotionLaunch L)
{
    extern __shared__ __attribute__((aligned(16))) unsigned motion_lds[];
    motion_key_t *const keys = (motion_key_t *)(motion_lds + MOTION_LDS_KEYS);
    unsigned *const blk = motion_lds + MOTION_LDS_BLOCK, *const cost = motion_lds + MOTION_LDS_COST, *const win = motion_lds + MOTION_LDS_WINDOW;
    const int tid = (int)threadIdx.x, nthreads = (int)blockDim.x;
    const int nmb = L.mb_cols * L.mb_rows, mb = (int)blockIdx.x, my = mb / L.mb_cols, mx = mb - my * L.mb_cols;
    const HistFrameJob J = L.j[blockIdx.y];
    const HistFrame C = frame_of(raster, fb_stride, tiles, tile_frame, J.fb), R = frame_of(raster, fb_stride, tiles, tile_frame, J.ref);
    const int d = L.d, pitch = L.pitch;

    // (everything down to the staging is the same for every lane)
    const int cmin = -(16 * mx + 16), cmax = 16 * (L.mb_cols - 1 - mx) + 16, rmin = -(16 * my + 16), rmax = 16 * (L.mb_rows - 1 - my) + 16;
    int cx = 0, cy = 0;
    if (L.centre) {
        const GLOBAL_AS short *cp = (const GLOBAL_AS short *)(centre + centre_stride * blockIdx.y);
        cx = cp[mb];
        cy = cp[nmb + mb];
    }
    cx = min(max(cx, cmin), cmax);
    cy = min(max(cy, rmin), rmax);
    const int x0 = 16 * mx + cx - d, y0 = 16 * my + cy - d;

    if (R.form == SCALE_FROM_RASTER) motion_stage<SCALE_FROM_RASTER>(win, R, L, x0, y0);
    else if (R.form == SCALE_FROM_TILES) motion_stage<SCALE_FROM_TILES>(win, R, L, x0, y0);
    else
        for (int i = tid; i < L.rows * pitch; i += nthreads) win[i] = 0u;
    if (tid < 64) blk[tid] = frame_read4<0>(C, L, 16 * mx + 4 * (tid & 3), 16 * my + (tid >> 2));
    if (L.spb)
        for (int i = tid; i < 2 * MOTION_COST_ROW; i += nthreads) cost[i] = L.cost[i / MOTION_COST_ROW][i % MOTION_COST_ROW];
    __syncthreads();

    motion_key_t best = MOTION_NEVER;
#pragma unroll 1
    for (int it = tid; it < L.groups * L.nq; it += nthreads) {
        const int g = it / L.nq, k = it - g * L.nq;
        const unsigned *w = win + g * MOTION_ROWS * pitch + k;
        unsigned long long acc[MOTION_ROWS];
#pragma unroll
        for (int t = 0; t < MOTION_ROWS; t++) acc[t] = 0;
        // A window row serves the block rows wr, wr - 1 .. wr - MOTION_ROWS + 1: those four block rows are in registers (slot = row
        // & 3), the next comes from LDS with the next window row -- every lane reads the same 16 bytes: a broadcast.  Reads run
        // one row ahead and no further
        unsigned v[5], next[5];
        u32x4_t brow[MOTION_ROWS], bnext = ((const u32x4_t *)blk)[0];
#pragma unroll
        for (int j = 0; j < 5; j++) next[j] = w[j];
#pragma unroll
        for (int wr = 0; wr < 15 + MOTION_ROWS; wr++) {
#pragma unroll
            for (int j = 0; j < 5; j++) v[j] = next[j];
            if (wr < 16) brow[wr % MOTION_ROWS] = bnext;
            if (wr + 1 < 15 + MOTION_ROWS) {
#pragma unroll
                for (int j = 0; j < 5; j++) next[j] = w[(wr + 1) * pitch + j];
                if (wr + 1 < 16) bnext = ((const u32x4_t *)blk)[wr + 1];
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int t = 0; t < MOTION_ROWS; t++) {
                const int br = wr - t;                // the block row this window row is for candidate row t of the item
                if (br < 0 || br > 15) continue;
#pragma unroll
                for (int j = 0; j < 4; j++)
                    acc[t] = __builtin_amdgcn_qsad_pk_u16_u8((unsigned long long)v[j + 1] << 32 | v[j], brow[br % MOTION_ROWS][j], acc[t]);
            }
            // all four sums stand here before the next window row is touched: without this the optimiser sinks three of the four
            // chains behind the loop and keeps every window row alive for them
            asm volatile("" : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3]));
        }
#pragma unroll
        for (int t = 0; t < MOTION_ROWS; t++) {
            const int ri = g * MOTION_ROWS + t, r = cy - d + ri;
            const bool rok = ri < 2 * d && r >= rmin && r < rmax;
            const unsigned cost_r = L.spb ? cost[ri] : 0u;        // (without a cost term the table was not staged)
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int ci = 4 * k + q, c = cx - d + ci;
                const bool at_centre = ri == d && ci == d;        // the centre is valued first and whatever the bounds are
                const bool ok = at_centre || (rok && ci < 2 * d && c >= cmin && c < cmax);
                unsigned value = (unsigned)(acc[t] >> (16 * q)) & 0xffffu;
                if (L.spb) value += ((cost_r + cost[MOTION_COST_ROW + ci]) * (unsigned)L.spb + 128u) >> 8;
                const unsigned order = at_centre ? 0u : 1u + (unsigned)(ri * 2 * d + ci);
                const motion_key_t key = ok ? (motion_key_t)value << 32 | order : MOTION_NEVER;
                best = key < best ? key : best;
            }
        }
    }

    best = motion_wave_min(best);
    if ((tid & 63) == 0) keys[tid >> 6] = best;
    __syncthreads();
    if (tid >= 64) return;
    motion_key_t key = keys[0];
    for (int wv = 1; wv < nthreads >> 6; wv++) key = keys[wv] < key ? keys[wv] : key;
    const unsigned order = (unsigned)key, value = (unsigned)(key >> 32);
    const int ri = order ? (int)((order - 1u) / (unsigned)(2 * d)) : d, ci = order ? (int)((order - 1u) % (unsigned)(2 * d)) : d;

    if (L.mv && tid == 0) {
        GLOBAL_AS short *o = (GLOBAL_AS short *)(mv + mv_stride * blockIdx.y);
        o[mb] = (short)((cx - d + ci) << 3);
        o[nmb + mb] = (short)((cy - d + ri) << 3);
    }
    if (!L.planes) return;

    const int row = tid >> 2, j = tid & 3;
    const unsigned s = blk[tid];
    const unsigned s1 = __builtin_amdgcn_udot4(s, 0x01010101u, 0u, false), ss = __builtin_amdgcn_udot4(s, s, 0u, false);
    unsigned sse = 0, sum = 0, sad0 = 0;
    if (L.planes & (MOTION_SSE | MOTION_VAR)) {
        const unsigned *wp = win + (ri + row) * pitch + (ci >> 2) + j;
        const unsigned r = __builtin_amdgcn_alignbyte(wp[1], wp[0], (unsigned)ci & 3u);
        // sum (s - r)^2 = ss - 2 sr + rr and sum (s - r) = s1 - r1, in wrapping arithmetic: the totals are below 2^32 / inside int32
        sse = ss + __builtin_amdgcn_udot4(r, r, 0u, false) - 2u * __builtin_amdgcn_udot4(s, r, 0u, false);
        sum = s1 - __builtin_amdgcn_udot4(r, 0x01010101u, 0u, false);
    }
    if (L.planes & MOTION_SAD0) sad0 = __builtin_amdgcn_sad_u8(s, frame_read4<0>(R, L, 16 * mx + 4 * j, 16 * my + row), 0u);
    sse = motion_wave_sum(sse);
    sum = motion_wave_sum(sum);
    sad0 = motion_wave_sum(sad0);
    const unsigned S1 = motion_wave_sum(s1), SS = motion_wave_sum(ss);
    if (tid) return;

    GLOBAL_AS unsigned *o = (GLOBAL_AS unsigned *)(stats + stats_stride * blockIdx.y) + mb;
    if (L.planes & MOTION_SAD) { *o = value; o += nmb; }
    if (L.planes & MOTION_SAD0) { *o = sad0; o += nmb; }
    if (L.planes & MOTION_SSE) { *o = sse; o += nmb; }
    if (L.planes & MOTION_VAR) {
        const long long sm = (long long)(int)sum;
        *o = sse - (unsigned)((sm * sm) >> 8);
        o += nmb;
    }
    if (L.planes & MOTION_SRCVAR) {
        // the block against the constant 128: sum (s - 128) and sum (s - 128)^2 from the block's own two sums
        const long long sm = (long long)S1 - 128 * 256;
        *o = SS - 256u * S1 + 128u * 128u * 256u - (unsigned)((sm * sm) >> 8);
    }
}
