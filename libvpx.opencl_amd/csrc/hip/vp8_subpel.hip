// Sub-pixel refinement of block motion between pictures (vp8hip_frames_subpel_async; vp8hip_subpel.hip has the plan, include/vp8hip.h
// the definition): per macroblock of frame buffer fb the step vp8_find_best_sub_pixel_step makes around a whole-pixel start into
// ref_fb -- eleven evaluations of vp8_sub_pixel_variance16x16_c in four dependent decisions (six evaluations in two for
// vp8_find_best_half_pixel_step) -- and what the result costs.  A WAVE owns one macroblock of one job; SUBPEL_WAVES of them share a
// workgroup and nothing else: no LDS, no barrier.  Nothing but the outputs is written.
//
// REGISTERS.  Lane l owns the four pixels of block row l >> 2 at columns 4 (l & 3) ..: its dword of the block, and the 3 rows x 6
// bytes of E(ref_fb) around them that the candidates can touch -- rows s - 1 .. s + 1 and columns s - 1 .. s + 4 of its own
// position s, read once as three aligned dwords a row through frame_edge4 (all clamps are spent there) and shifted together
// (the shift is the start's column & 3: the same for every lane).  A row is kept as the three dwords of columns -1 .., 0 .., +1 ..
// PREDICTION.  A candidate is (dy, dx) in 1/8 pel against v0 = 8 * start, each of -6 .. 6 and even.  Its base is -1 where the
// component is negative, else 0, and its offset the component & 7: which two of the three dwords / rows it filters.  The
// reference's taps are {128 - 16 o, 16 o} with + 64 >> 7: all multiples of 16, so (a (8 - o) + b o + 4) >> 3 gives the same bits,
// below 2^11 -- two pixels go through one multiply in the halves of a dword.  Both passes are always made, the first rounded before
// the second, as the reference does; the offset 0 passes its input through.
// SUMS.  sum (s - p)^2 = ss - 2 sp + pp and sum (s - p) = s1 - p1 from v_dot4_u32_u8 on the four predicted bytes, per lane; a wave's
// total by four DPP adds inside a row of 16 lanes and v_readlane of the four rows: the totals are scalars, so the four decisions --
// the strict <, the diagonal, the second stage's centre -- are made once per wave, and no lane branches on anything else.  The
// evaluations of a stage's first part are independent of each other and their reductions interleave.
#include "vp8_frame_read.hip.h"
#include "vp8hip.h"

// a wave's total of v, the same in every lane (all 64 lanes are active)
__device__ __forceinline__ unsigned subpel_wave_sum(unsigned v)
{
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false);       // quad_perm [1, 0, 3, 2]
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false);       // quad_perm [2, 3, 0, 1]
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, false);      // row_half_mirror: the other quad of eight
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, false);      // row_mirror: the other eight of the row
    return (unsigned)__builtin_amdgcn_readlane((int)v, 0) + (unsigned)__builtin_amdgcn_readlane((int)v, 16) +
           (unsigned)__builtin_amdgcn_readlane((int)v, 32) + (unsigned)__builtin_amdgcn_readlane((int)v, 48);
}

// one filter pass over two pixels in each of `a` and `b` (a byte in every half): (a (8 - o) + b o + 4) >> 3 per half.  At offset 0
// that is (8 a + 4) >> 3 = a: the pass is made by handing its input on -- in the first stage, whose offsets are constants, the
// compiler drops the arithmetic and the row it no longer reads; in the second o is the same for every lane
__device__ __forceinline__ unsigned subpel_tap(unsigned a, unsigned b, unsigned o)
{
    if (o == 0u) return a;
    return ((a * (8u - o) + b * o + 0x00040004u) >> 3) & 0x00ff00ffu;
}

struct SubpelWindow {
    unsigned m[3], z[3], p[3];        // rows -1, 0, +1 of the lane's position: the dwords that begin at columns -1, 0, +1
};

// the lane's four predicted bytes of the candidate (dy, dx) (the same for every lane)
__device__ __forceinline__ unsigned subpel_predict(const SubpelWindow &W, int dy, int dx)
{
    const unsigned ox = (unsigned)dx & 7u, oy = (unsigned)dy & 7u;
    const int top = dy < 0 ? 0 : 1;
    unsigned h[2][2];                                 // [top, bottom][even, odd pixels] after the horizontal pass
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const unsigned rm = top + i == 0 ? W.m[0] : top + i == 1 ? W.m[1] : W.m[2];
        const unsigned rz = top + i == 0 ? W.z[0] : top + i == 1 ? W.z[1] : W.z[2];
        const unsigned rp = top + i == 0 ? W.p[0] : top + i == 1 ? W.p[1] : W.p[2];
        const unsigned a = dx < 0 ? rm : rz, b = dx < 0 ? rz : rp;
        h[i][0] = subpel_tap(a & 0x00ff00ffu, b & 0x00ff00ffu, ox);
        h[i][1] = subpel_tap((a >> 8) & 0x00ff00ffu, (b >> 8) & 0x00ff00ffu, ox);
    }
    return subpel_tap(h[0][0], h[1][0], oy) | subpel_tap(h[0][1], h[1][1], oy) << 8;
}

// what a lane adds to a candidate's sums
struct SubpelPart {
    unsigned sse;                     // sum (s - p)^2 of its four pixels
    unsigned sum;                     // sum (s - p), two's complement
};

__device__ __forceinline__ SubpelPart subpel_part(unsigned s, unsigned s1, unsigned ss, unsigned p)
{
    return SubpelPart{ss + __builtin_amdgcn_udot4(p, p, 0u, false) - 2u * __builtin_amdgcn_udot4(s, p, 0u, false),
                      s1 - __builtin_amdgcn_udot4(p, 0x01010101u, 0u, false)};
}

// a candidate valued (everything here is the same for every lane)
struct SubpelCand {
    unsigned val, var, sse;
    int dy, dx;
};

template <int FORM>
__device__ __forceinline__ void subpel_load(SubpelWindow &W, const HistFrame &R, const FramePlanes &L, int px, int py)
{
    const int xa = px & ~3;
    const unsigned sh = (unsigned)px & 3u;            // (the same for every lane: a lane's px is the start's column + 4 k - 1)
    unsigned w[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int k = 0; k < 3; k++) w[i][k] = frame_edge4<FORM>(R, L, xa + 4 * k, py + i);
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const unsigned lo = __builtin_amdgcn_alignbyte(w[i][1], w[i][0], sh), hi = __builtin_amdgcn_alignbyte(w[i][2], w[i][1], sh);
        W.m[i] = lo;
        W.z[i] = __builtin_amdgcn_alignbyte(hi, lo, 1u);
        W.p[i] = __builtin_amdgcn_alignbyte(hi, lo, 2u);
    }
}

// grid: x = the macroblocks in raster order, SUBPEL_WAVES a workgroup, y = the jobs of the launch; 64 * SUBPEL_WAVES threads, no LDS.
// raster / tiles: frame buffer 0 in its two forms (vp8_scale_kernel's); start / ref / mv / stats: the launch's first tensors (null
// where L says there is none); cost: the context's copy of the table, [2][2 R + 1] (not read where L.epb is 0)
extern "C" __global__ void __launch_bounds__(64 * SUBPEL_WAVES)
vp8_subpel_frames_kernel(const uint8_t *__restrict__ raster, size_t fb_stride, const uint8_t *__restrict__ tiles, size_t tile_frame,
                         const uint8_t *__restrict__ start, size_t start_stride, const uint8_t *__restrict__ ref, size_t ref_stride,
                         uint8_t *__restrict__ mv, size_t mv_stride, uint8_t *__restrict__ stats, size_t stats_stride,
                         const unsigned short *__restrict__ cost, SubpelLaunch L)
{
    const int lane = (int)threadIdx.x & 63;
    const int nmb = L.mb_cols * L.mb_rows;
    // (the wave's number as a scalar: everything down to the loads is the same for every lane)
    const int mb = (int)blockIdx.x * SUBPEL_WAVES + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    if (mb >= nmb) return;
    const int my = mb / L.mb_cols, mx = mb - my * L.mb_cols;
    const HistFrameJob J = L.j[blockIdx.y];
    const HistFrame C = frame_of(raster, fb_stride, tiles, tile_frame, J.fb), R = frame_of(raster, fb_stride, tiles, tile_frame, J.ref);

    const int cmin = -(16 * mx + 16), cmax = 16 * (L.mb_cols - 1 - mx) + 16, rmin = -(16 * my + 16), rmax = 16 * (L.mb_rows - 1 - my) + 16;
    int sx = 0, sy = 0, rx = 0, ry = 0;
    if (L.start) {
        const GLOBAL_AS short *sp = (const GLOBAL_AS short *)(start + start_stride * blockIdx.y);
        sx = sp[mb] >> 3;
        sy = sp[nmb + mb] >> 3;
    }
    sx = min(max(sx, cmin), cmax);
    sy = min(max(sy, rmin), rmax);
    if (L.epb && L.ref) {
        const GLOBAL_AS short *rp = (const GLOBAL_AS short *)(ref + ref_stride * blockIdx.y);
        rx = rp[mb];
        ry = rp[nmb + mb];
    }

    const int row = lane >> 2, q = lane & 3;
    const unsigned s = frame_read4<0>(C, L, 16 * mx + 4 * q, 16 * my + row);
    SubpelWindow W;
    const int px = 16 * mx + sx + 4 * q - 1, py = 16 * my + sy + row - 1;
    if (R.form == SCALE_FROM_RASTER) subpel_load<SCALE_FROM_RASTER>(W, R, L, px, py);
    else if (R.form == SCALE_FROM_TILES) subpel_load<SCALE_FROM_TILES>(W, R, L, px, py);
    else
#pragma unroll
        for (int i = 0; i < 3; i++) W.m[i] = W.z[i] = W.p[i] = 0u;
    const unsigned s1 = __builtin_amdgcn_udot4(s, 0x01010101u, 0u, false), ss = __builtin_amdgcn_udot4(s, s, 0u, false);

    // a candidate's value from its two totals: DIST + COST
    const int Rr = L.R, vy0 = 8 * sy - ry, vx0 = 8 * sx - rx;
    auto valued = [&](SubpelPart t, int dy, int dx) {
        const long long sm = (long long)(int)t.sum;
        const unsigned var = t.sse - (unsigned)((sm * sm) >> 8);
        unsigned c = 0u;
        if (L.epb) {
            const int iy = min(max((vy0 + dy) >> 1, -Rr), Rr) + Rr, ix = min(max((vx0 + dx) >> 1, -Rr), Rr) + Rr;
            c = (((unsigned)cost[iy] + (unsigned)cost[2 * Rr + 1 + ix]) * (unsigned)L.epb + 128u) >> 8;
        }
        return SubpelCand{var + c, var, t.sse, dy, dx};
    };
    auto total = [&](SubpelPart t) { return SubpelPart{subpel_wave_sum(t.sse), subpel_wave_sum(t.sum)}; };
    auto part = [&](int dy, int dx) { return subpel_part(s, s1, ss, subpel_predict(W, dy, dx)); };

    // the centre: the whole-pixel block itself
    const SubpelPart t0 = part(0, 0);
    SubpelCand best = {};
    unsigned var0 = 0u;
    int cy = 0, cx = 0;
#pragma unroll
    for (int h = 4; h >= 2; h -= 2) {
        if (h == 2 && L.precision != 4) break;
        // left, right, up, down around (cy, cx), the lanes' parts first, then the totals: the reductions do not wait for each other
        const SubpelPart pl = part(cy, cx - h), pr = part(cy, cx + h), pu = part(cy - h, cx), pd = part(cy + h, cx);
        if (h == 4) {
            best = valued(total(t0), 0, 0);
            var0 = best.var;
        }
        const SubpelCand left = valued(total(pl), cy, cx - h), right = valued(total(pr), cy, cx + h);
        const SubpelCand up = valued(total(pu), cy - h, cx), down = valued(total(pd), cy + h, cx);
        if (left.val < best.val) best = left;
        if (right.val < best.val) best = right;
        if (up.val < best.val) best = up;
        if (down.val < best.val) best = down;
        const int ddx = left.val < right.val ? -h : h, ddy = up.val < down.val ? -h : h;
        const SubpelCand diag = valued(total(part(cy + ddy, cx + ddx)), cy + ddy, cx + ddx);
        if (diag.val < best.val) best = diag;
        cy = best.dy;
        cx = best.dx;
    }

    if (lane) return;
    if (L.mv) {
        GLOBAL_AS short *o = (GLOBAL_AS short *)(mv + mv_stride * blockIdx.y);
        o[mb] = (short)(8 * sx + best.dx);
        o[nmb + mb] = (short)(8 * sy + best.dy);
    }
    if (!L.planes) return;
    GLOBAL_AS unsigned *o = (GLOBAL_AS unsigned *)(stats + stats_stride * blockIdx.y) + mb;
    if (L.planes & SUBPEL_VAL) { *o = best.val; o += nmb; }
    if (L.planes & SUBPEL_VAR) { *o = best.var; o += nmb; }
    if (L.planes & SUBPEL_SSE) { *o = best.sse; o += nmb; }
    if (L.planes & SUBPEL_VAR0) *o = var0;
}

// the cost table on its way to the context's copy: a piece of it comes with the launch, so the caller's memory is read at the call
// and never later, and the copy is ordered on the stream like the kernel that reads it.  grid: 1; SUBPEL_TABLE_PIECE threads at most
extern "C" __global__ void __launch_bounds__(256) vp8_subpel_table_kernel(unsigned short *__restrict__ dst, SubpelTablePiece P)
{
    for (int i = (int)threadIdx.x; i < P.n; i += (int)blockDim.x) dst[P.first + i] = P.v[i];
}
