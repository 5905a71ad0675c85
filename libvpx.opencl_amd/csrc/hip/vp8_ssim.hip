// Structural similarity of picture pairs (vp8hip_frames_ssim_async; vp8hip_ssim.hip has the plan, include/vp8hip.h the definition):
// vp8_ssim2's 8x8 windows on the 4-pixel grid over the display-size planes of two frame buffers, each read in the form it has, as a
// Q32 total per plane and as a map of the window values.  A stencil and a reduction; the library's one kernel on the f64 pipe.
//
// CELLS.  A window is 2 x 2 cells of 4 x 4 samples and neighbouring windows share cells, so a cell's five sums are made once: a
// lane reads the cell's four rows of either picture as aligned dwords (frame_read4, vp8_frame_read.hip.h: cells are dword-aligned
// and lie inside the display width, there are no partial cells) and takes the byte dot product of each dword with itself, with
// the other picture's and with 0x01010101.  The sums go to LDS as one 16-byte piece: sum s | sum r << 16 (at most 16 * 255 each),
// sum ss, sum rr, sum sr (at most 16 * 255^2 each).
// PIECES.  A workgroup stages the cells of a piece -- SSIM_BAND_ROWS window rows of a band by SSIM_BAND_COLS window columns, plus
// one halo cell row and one halo cell column, which are read and not owned: a window belongs to the piece of its top left cell --
// and then takes a lane per window: four cells added, the two 64-bit products of similarity(), one conversion each, one division,
// and for the scores the product with 2^32 rounded to the nearest integer, half to even.  Nothing else is done in floating point
// and none of it is a multiply feeding an add, so there is nothing to contract or reassociate: the value is the same bits as
// (double)n / (double)d anywhere IEEE arithmetic is.
// REDUCTION.  A lane sums its windows' Q32 values per plane in an int64, the wave adds its lanes', the workgroup its waves' in
// LDS; then one 16-byte store {total, count} per plane where the workgroup owns the job (gridDim.x == 1), else --
// vp8_ssim_fill_kernel has written {0, count} on the same stream -- one 64-bit global atomic add without return per plane.  Integer
// adds commute: the same bits in every run, whatever order lanes and workgroups arrive in.  The count is the plan's arithmetic.
// MAP.  A lane stores its window's element; the lanes of a wave lie on neighbouring windows of a row.  Every element is written
// once, by the piece that owns the window.  Nothing but the outputs is written.
#include <hip/hip_fp16.h>
#include "vp8_frame_read.hip.h"
#include "vp8_tensor_out.hip.h"
#include "vp8hip.h"

#pragma clang fp contract(off)

#define SSIM_CELL_COLS (SSIM_BAND_COLS + 1)
#define SSIM_CELL_ROWS (SSIM_BAND_ROWS + 1)

// grid: x = 1, y = the jobs of the launch.  dst: the launch's first scores
extern "C" __global__ void __launch_bounds__(64) vp8_ssim_fill_kernel(uint8_t *dst, size_t dst_stride, SsimFill F)
{
    if ((int)threadIdx.x < F.np) {
        GLOBAL_AS long long *o = (GLOBAL_AS long long *)(dst + dst_stride * blockIdx.y) + 2 * threadIdx.x;
        o[0] = 0;
        o[1] = F.count[threadIdx.x];
    }
}

// the five sums of the cell at (x, y) of plane PL
template <int PL>
__device__ __forceinline__ u32x4_t ssim_cell(const HistFrame &C, const HistFrame &R, const SsimLaunch &L, int x, int y)
{
    unsigned s[4], r[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {                // (all eight loads in flight before the first dot product)
        s[i] = frame_read4<PL>(C, L, x, y + i);
        r[i] = frame_read4<PL>(R, L, x, y + i);
    }
    unsigned ss = 0, rr = 0, sr = 0, s1 = 0, r1 = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        ss = __builtin_amdgcn_udot4(s[i], s[i], ss, false);
        rr = __builtin_amdgcn_udot4(r[i], r[i], rr, false);
        sr = __builtin_amdgcn_udot4(s[i], r[i], sr, false);
        s1 = __builtin_amdgcn_udot4(s[i], 0x01010101u, s1, false);
        r1 = __builtin_amdgcn_udot4(r[i], 0x01010101u, r1, false);
    }
    return u32x4_t{s1 | r1 << 16, ss, rr, sr};
}

// the cells of a piece into LDS: rows cy0 .. cy0 + nrows - 1, columns cx0 .. cx0 + ncols - 1 of plane PL's cell grid
template <int PL>
__device__ __forceinline__ void ssim_stage(u32x4_t *cells, const HistFrame &C, const HistFrame &R, const SsimLaunch &L, int cx0, int cy0, int ncols,
                                           int nrows)
{
#pragma unroll 1
    for (TensorWalk t(ncols); t.row < nrows; t.next())
        cells[t.row * SSIM_CELL_COLS + t.col] = ssim_cell<PL>(C, R, L, 4 * (cx0 + t.col), 4 * (cy0 + t.row));
}

// similarity() with count 64 over the sums of a window (four cells added): n / d
__device__ __forceinline__ double ssim_value(const u32x4_t &w)
{
    const int c1 = 26634, c2 = 239708;
    const int s = (int)(w.x & 0xffffu), r = (int)(w.x >> 16);          // at most 64 * 255 each
    const int sr2 = 2 * s * r, sq = s * s + r * r;                       // at most 2 * 16320^2 < 2^29.99
    const long long n = (long long)(sr2 + c1) * (long long)(128 * (int)w.w - sr2 + c2);
    const long long d = (long long)(sq + c1) * (long long)(64 * (int)(w.y + w.z) - sq + c2);
    return (double)n / (double)d;
}

// a wave's sum in its lane 0
__device__ __forceinline__ long long ssim_wave_sum(long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// grid: x = the workgroups that share a job's pieces (L.S), y = the jobs of the launch.  raster / tiles: frame buffer 0 in its two
// forms (vp8_scale_kernel's); scores / map: the launch's first outputs (null where L says there is none)
extern "C" __global__ void __launch_bounds__(256)
vp8_ssim_frames_kernel(const uint8_t *__restrict__ raster, size_t fb_stride, const uint8_t *__restrict__ tiles, size_t tile_frame,
                       uint8_t *__restrict__ scores, size_t scores_stride, uint8_t *__restrict__ map, size_t map_stride, SsimLaunch L)
{
    __shared__ u32x4_t cells[SSIM_CELL_ROWS * SSIM_CELL_COLS];
    __shared__ long long wave_sum[4][3];
    const HistFrameJob J = L.j[blockIdx.y];
    const HistFrame C = frame_of(raster, fb_stride, tiles, tile_frame, J.fb), R = frame_of(raster, fb_stride, tiles, tile_frame, J.ref);
    uint8_t *const m = map + map_stride * blockIdx.y;
    long long acc[3] = {0, 0, 0};

#pragma unroll 1
    for (int piece = (int)blockIdx.x; piece < L.pieces; piece += (int)gridDim.x) {
        // (everything here is the same for every lane)
        const int k = L.np > 2 && piece >= L.p[2].first ? 2 : L.np > 1 && piece >= L.p[1].first ? 1 : 0;
        const SsimPlane P = L.p[k];
        const int q = piece - P.first, band = q / P.px, strip = q - band * P.px;
        const int wx0 = strip * SSIM_BAND_COLS, wy0 = band * SSIM_BAND_ROWS;
        const int nx = min(SSIM_BAND_COLS, P.nwx - wx0), ny = min(SSIM_BAND_ROWS, P.nwy - wy0);
        __syncthreads();                                   // the piece before has been read
        if (P.pl == 0) ssim_stage<0>(cells, C, R, L, wx0, wy0, nx + 1, ny + 1);
        else if (P.pl == 1) ssim_stage<1>(cells, C, R, L, wx0, wy0, nx + 1, ny + 1);
        else ssim_stage<2>(cells, C, R, L, wx0, wy0, nx + 1, ny + 1);
        __syncthreads();
        long long sum = 0;
#pragma unroll 1
        for (TensorWalk t(nx); t.row < ny; t.next()) {
            const u32x4_t *c = cells + t.row * SSIM_CELL_COLS + t.col;
            const u32x4_t w = c[0] + c[1] + c[SSIM_CELL_COLS] + c[SSIM_CELL_COLS + 1];      // (the packed halves cannot carry: 64 * 255 < 2^16)
            const double v = ssim_value(w);
            if (L.scores) sum += (long long)__builtin_rint(v * 4294967296.0);
            if (L.map_dtype) {
                const size_t e = (size_t)P.map_off + (size_t)(wy0 + t.row) * (size_t)P.nwx + (size_t)(wx0 + t.col);
                const float f = (float)v;
                if (L.map_dtype == SSIM_F32) ((GLOBAL_AS float *)m)[e] = f;
                else ((GLOBAL_AS unsigned short *)m)[e] = __half_as_ushort(__float2half_rn(f));
            }
        }
        if (k == 0) acc[0] += sum;
        else if (k == 1) acc[1] += sum;
        else acc[2] += sum;
    }
    if (!L.scores) return;

    const int wave = (int)(threadIdx.x >> 6);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const long long s = ssim_wave_sum(acc[k]);
        if ((threadIdx.x & 63u) == 0) wave_sum[wave][k] = s;
    }
    __syncthreads();
    if ((int)threadIdx.x < L.np) {
        const int k = (int)threadIdx.x;
        const long long total = wave_sum[0][k] + wave_sum[1][k] + wave_sum[2][k] + wave_sum[3][k];
        GLOBAL_AS long long *o = (GLOBAL_AS long long *)(scores + scores_stride * blockIdx.y) + 2 * k;
        if (gridDim.x == 1) {
            typedef long long i64x2_t __attribute__((ext_vector_type(2), aligned(8)));       // (scores are aligned to 8)
            *(GLOBAL_AS i64x2_t *)o = i64x2_t{total, (long long)L.p[k].nwx * L.p[k].nwy};
        } else if (total) {
            (void)__hip_atomic_fetch_add(o, total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}
