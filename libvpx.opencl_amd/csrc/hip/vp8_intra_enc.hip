// Intra modes and levels of key-frame macroblocks (vp8hip_frames_intra_async; vp8hip_intra.hip has the plan, include/vp8hip.h the
// definition): the reference's vp8_pick_intra_mode followed by the body of vp8cx_encode_intra_macro_block, per macroblock.
//
// A macroblock is predicted from the reconstruction of its left, above-left, above and above-right neighbours, so a picture is a
// wavefront: step s holds the macroblocks (r, c) with c + 2 r == s.  A WORKGROUP owns one job and walks the steps with a workgroup
// barrier between them; the INTRA_WAVES waves take the macroblocks of a step in turn, a WAVE a macroblock.  Nothing waits on a flag
// and nothing is shared between workgroups: the device is filled with jobs.  No atomics: the same bits in every run.
//
// NEIGHBOURS live in LDS only as long as they are read.  The bottom line of (r, c) -- Y 16, U 8, V 8 pixels and the four sub-block
// modes of its bottom block row -- is written at step s and read by (r + 1, c - 1), (r + 1, c) and (r + 1, c + 1) at steps s + 1
// .. s + 3: a ring of four lines per row, slot c & 3 (the writer of a step is four columns ahead of the oldest reader's slot, never
// on it).  The right column of (r, c) is read by (r, c + 1) a step later: one per row.  Rows are walked in BANDS of INTRA_BAND
// rows, so the rings are as many; the last row of a band that has a successor also leaves its lines in a line of the picture's
// width (dynamic LDS, only where the picture has more rows than a band), which the first row of the next band reads.
//
// INSIDE A MACROBLOCK the wave first builds the decoder's borders around a 16x16 luma frame and two 8x8 chroma frames in its own LDS
// (127 above the picture, 129 to its left, the above-right of the last column the line's last pixel).  Then
//   CHROMA MODE  a lane a pixel of U and of V: the four squared errors, summed over the wave;
//   16x16 MODE   a lane four pixels of a row: sum and squared error of the four predictions, summed over the wave;
//   B_PRED       sixteen serial blocks.  Lane 16 m + p makes pixel p of mode m0 + m from the block's edge vector (k_bpred_tab): four
//                modes a round, their errors summed over sixteen lanes.  The block's fdct, quantiser scan and inverse transform run
//                in lane 0 (the scan is serial anyway); sixteen lanes add and store the reconstruction, the next block's neighbour.
//   BLOCKS       vp8_quant.hip's block phase: lane b < 24 owns block b (luma only where a 16x16 mode won), lane 24 the Y2 block.
// and the lines for the neighbours and the outputs are written.  Every lane of a wave meets every wave-level fence.
#include "vp8_frame_read.hip.h"
#include "vp8_block_prims.hip.h"
#include "vp8_quant_prims.hip.h"
#include "vp8hip.h"

static_assert(INTRA_RD16 == VP8HIP_INTRA_RD16 && INTRA_RD4 == VP8HIP_INTRA_RD4 && INTRA_RATE == VP8HIP_INTRA_RATE, "");
static_assert(INTRA_EOBS == VP8HIP_INTRA_EOBS && INTRA_RECSSE == VP8HIP_INTRA_RECSSE, "");
static_assert(QUANT_TABLE_SHORTS == 88 && INTRA_THREADS >= 500, "");

#define FY_STRIDE 24              // the luma frame: rows -1 .. 15, a row = columns -4 .. 19 (column -1 at byte 3, dwords aligned)
#define FC_STRIDE 12              // a chroma frame: rows -1 .. 7, a row = columns -4 .. 7
#define INTRA_INT_MAX 0x7fffffff

struct IntraWave {                // a wave's own LDS
    u32 src[96];                  // the source: Y dword 4 row + g, U 64 + 2 row + g, V 80 + 2 row + g
    __attribute__((aligned(4))) uint8_t fy[17 * FY_STRIDE];
    __attribute__((aligned(4))) uint8_t fc[2][9 * FC_STRIDE];
    __attribute__((aligned(4))) short res[16];        // a sub-block's residual, then what its inverse transform adds
    __attribute__((aligned(4))) short dcs[16];        // the luma blocks' coefficient 0, later their Walsh DC
    __attribute__((aligned(4))) short blev[16 * 16];  // B_PRED: what coef holds of the sixteen blocks
    __attribute__((aligned(4))) uint8_t beob[16], bm[16], P[16];
};

__device__ __forceinline__ int rdcost(int rdmult, int rddiv, int rate, int dist) { return ((128 + rate * rdmult) >> 8) + rddiv * dist; }
__device__ __forceinline__ int sq_diff4(u32 s, u32 p, int &sum)
{
    int e = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int t = (int)((s >> (8 * i)) & 0xffu) - (int)((p >> (8 * i)) & 0xffu);
        sum += t;
        e += t * t;
    }
    return e;
}

// pixel px (4 row + column) of vp8_intra4x4_predict's mode m over the edge vector P = {L3 L3 L2 L1 L0 TL A0 .. A7 A7}
__device__ __forceinline__ int bpred_pixel(const uint8_t *P, const uint8_t *btab, int m, int px)
{
    const int e = btab[16 * m + px], kind = e >> 4, k = e & 15;
    const int a = P[k ? k - 1 : 0], b = P[k], c = P[k + 1];
    const int dc = (P[1] + P[2] + P[3] + P[4] + P[6] + P[7] + P[8] + P[9] + 4) >> 3;
    const int tm = clamp255(P[4 - (px >> 2)] + P[6 + (px & 3)] - P[5]);
    const int dir = kind == 2 ? (a + 2 * b + c + 2) >> 2 : kind == 1 ? (b + c + 1) >> 1 : b;
    return m == VP8IR_B_DC_PRED ? dc : m == VP8IR_B_TM_PRED ? tm : dir;
}

// grid: x = the jobs of the launch; INTRA_THREADS threads; dynamic LDS: INTRA_LINE_WORDS dwords a macroblock column where the picture
// has more than INTRA_BAND rows.  raster / tiles: frame buffer 0 in its two forms; the five outputs: the launch's first job's
extern "C" __global__ void __launch_bounds__(INTRA_THREADS)
vp8_intra_enc_kernel(const uint8_t *__restrict__ raster, size_t fb_stride, const uint8_t *__restrict__ tiles, size_t tile_frame,
                     uint8_t *__restrict__ coef, size_t coef_stride, uint8_t *__restrict__ eobs, size_t eob_stride,
                     uint8_t *__restrict__ stats, size_t stats_stride, uint8_t *__restrict__ rec, size_t rec_stride,
                     uint8_t *__restrict__ modes, size_t modes_stride, IntraLaunch L)
{
    __shared__ __attribute__((aligned(16))) short tab[QUANT_TABLE_SHORTS];
    __shared__ __attribute__((aligned(4))) unsigned short bcost[1000];
    __shared__ __attribute__((aligned(4))) uint8_t btab[160];
    __shared__ u32 ring[INTRA_BAND][4][INTRA_LINE_WORDS], rcol[INTRA_BAND][INTRA_LINE_WORDS];
    __shared__ IntraWave waves[INTRA_WAVES];
    extern __shared__ u32 bound[];                                   // [mb_cols][INTRA_LINE_WORDS]
    const int tid = (int)threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int job = (int)blockIdx.x, cols = L.mb_cols, rows = L.mb_rows, nmb = cols * rows;
    const int jw = L.j[job];
    const HistFrame C = frame_of(raster, fb_stride, tiles, tile_frame, jw & 0x0fffffff);
    if (tid < QUANT_TABLE_SHORTS / 2) ((u32 *)tab)[tid] = ((const u32 *)L.t[(jw >> 28) & 3])[tid];
    if (tid < 500) ((u32 *)bcost)[tid] = ((const u32 *)L.bmode_cost)[tid];
    if (tid < 160) btab[tid] = k_bpred_tab[tid];
    __syncthreads();
    IntraWave &W = waves[wave];
    const int px = lane & 15;

    for (int r0 = 0; r0 < rows; r0 += INTRA_BAND) {
        const int nr = min(INTRA_BAND, rows - r0);
        const bool leave = r0 + nr < rows;                           // the band has a successor
        const int nsteps = cols + 2 * (nr - 1);
        for (int s = 0; s < nsteps; s++) {
            const int lo = max(0, (s - cols + 2) >> 1), hi = min(nr - 1, s >> 1);
            for (int rb = lo + wave; rb <= hi; rb += INTRA_WAVES) {
                const int r = r0 + rb, c = s - 2 * rb, mb = r * cols + c;
                const bool up = r > 0, lf = c > 0;
                // word w of the bottom line of (r - 1, cc)
                auto line = [&](int cc, int w) -> u32 { return rb == 0 ? bound[cc * INTRA_LINE_WORDS + w] : ring[rb - 1][cc & 3][w]; };

                // ---- the source and the borders
                W.src[lane] = frame_read4<0>(C, L, 16 * c + 4 * (lane & 3), 16 * r + (lane >> 2));
                if (lane < 32) {
                    const int x = 8 * c + 4 * (lane & 1), y = 8 * r + ((lane & 15) >> 1);
                    W.src[64 + lane] = lane < 16 ? frame_read4<1>(C, L, x, y) : frame_read4<2>(C, L, x, y);
                }
                if (lane < 4) *(u32 *)(W.fy + 4 + 4 * lane) = up ? line(c, lane) : 0x7f7f7f7fu;
                else if (lane == 4) *(u32 *)(W.fy + 20) = !up ? 0x7f7f7f7fu : c == cols - 1 ? (line(c, 3) >> 24) * 0x01010101u : line(c + 1, 0);
                else if (lane == 5) {                                // the three top-left pixels
                    W.fy[3] = (uint8_t)(!up ? 127u : !lf ? 129u : line(c - 1, 3) >> 24);
                    W.fc[0][3] = (uint8_t)(!up ? 127u : !lf ? 129u : line(c - 1, 5) >> 24);
                    W.fc[1][3] = (uint8_t)(!up ? 127u : !lf ? 129u : line(c - 1, 7) >> 24);
                } else if (lane < 10) {
                    const int k = lane - 6;                          // U: 0, 1; V: 2, 3
                    *(u32 *)(W.fc[k >> 1] + 4 + 4 * (k & 1)) = up ? line(c, 4 + k) : 0x7f7f7f7fu;
                } else if (lane >= 16 && lane < 32)
                    W.fy[(lane - 15) * FY_STRIDE + 3] = lf ? ((const uint8_t *)rcol[rb])[lane - 16] : (uint8_t)129;
                else if (lane >= 32 && lane < 48) {
                    const int k = lane - 32;                         // U: 0 .. 7; V: 8 .. 15
                    W.fc[k >> 3][((k & 7) + 1) * FC_STRIDE + 3] = lf ? ((const uint8_t *)rcol[rb])[16 + k] : (uint8_t)129;
                }
                const u32 ctx_above = up ? line(c, 8) : 0u, ctx_left = lf ? rcol[rb][8] : 0u;     // (B_DC_PRED is 0)
                compiler_fence();

                // ---- 1. the chroma mode
                int uv_mode = 0;
                int dcs[2] = {128, 128};
                {
                    const int row = lane >> 3, col = lane & 7;
                    if (up || lf) {
                        const int sh = 2 + up + lf;
#pragma unroll
                        for (int pl = 0; pl < 2; pl++) {
                            int v = 0;
                            if (lane < 8) v = (up ? W.fc[pl][4 + lane] : 0) + (lf ? W.fc[pl][(lane + 1) * FC_STRIDE + 3] : 0);
                            dcs[pl] = (wave_sum(v) + (1 << (sh - 1))) >> sh;
                        }
                    }
                    int e[4] = {0, 0, 0, 0};
#pragma unroll
                    for (int pl = 0; pl < 2; pl++) {
                        const int sp = ((const uint8_t *)W.src)[256 + 64 * pl + lane];
                        const int a = W.fc[pl][4 + col], l = W.fc[pl][(row + 1) * FC_STRIDE + 3], tl = W.fc[pl][3];
                        const int p[4] = {dcs[pl], a, l, clamp255(l + a - tl)};
#pragma unroll
                        for (int m = 0; m < 4; m++) e[m] += (sp - p[m]) * (sp - p[m]);
                    }
                    int best = INTRA_INT_MAX;
#pragma unroll
                    for (int m = 0; m < 4; m++) {
                        const int t = wave_sum(e[m]);
                        if (best > t) { best = t; uv_mode = m; }
                    }
                }

                // ---- 2. the 16x16 mode
                int ymode = 0, rd16 = INTRA_INT_MAX, best_sse = 0, best_rate = 0, dcy = 128;
                {
                    if (up || lf) {
                        const int sh = 3 + up + lf;
                        int v = 0;
                        if (lane < 16) v = (up ? W.fy[4 + lane] : 0) + (lf ? W.fy[(lane + 1) * FY_STRIDE + 3] : 0);
                        dcy = (wave_sum(v) + (1 << (sh - 1))) >> sh;
                    }
                    const u32 sp = W.src[lane], above = *(const u32 *)(W.fy + 4 + 4 * (lane & 3));
                    const int left = W.fy[((lane >> 2) + 1) * FY_STRIDE + 3], tl = W.fy[3];
#pragma unroll
                    for (int m = 0; m < 4; m++) {
                        int sum = 0;
                        int sse = sq_diff4(sp, intra_pred4(m, above, left, tl, dcy), sum);
                        sum = wave_sum(sum);
                        sse = wave_sum(sse);
                        const int var = (int)((u32)sse - (((u32)sum * (u32)sum) >> 8));
                        const int rate = L.mbmode_cost[m], rd = rdcost(L.rdmult, L.rddiv, rate, var);
                        if (rd16 > rd) { rd16 = rd; ymode = m; best_sse = sse; best_rate = rate; }
                    }
                }

                // ---- 3. B_PRED: sixteen dependent blocks
                int rd4 = INTRA_INT_MAX, cost = L.mbmode_cost[4];
                if (!L.no_bpred) {
                    int dist = 0, b = 0;
                    for (; b < 16; b++) {
                        const int by = b >> 2, bx = b & 3;
                        if (lane < 15) {                             // the edge vector
                            const int k = lane;
                            int at;
                            if (k < 5) at = (4 * by + 1 + (k < 2 ? 3 : 4 - k)) * FY_STRIDE + 3 + 4 * bx;
                            else if (k == 5) at = 4 * by * FY_STRIDE + 3 + 4 * bx;
                            else {
                                const int i = min(k, 13) - 6;        // above 0 .. 7; the right-hand block column takes the macroblock's above-right
                                at = (i >= 4 && bx == 3 ? 0 : 4 * by * FY_STRIDE) + 4 + 4 * bx + i;
                            }
                            W.P[k] = W.fy[at];
                        }
                        compiler_fence();
                        const int ctxA = by == 0 ? (int)((ctx_above >> (8 * bx)) & 0xffu) : (int)W.bm[b - 4];
                        const int ctxL = bx == 0 ? (int)((ctx_left >> (8 * by)) & 0xffu) : (int)W.bm[b - 1];
                        const unsigned short *bc = bcost + (ctxA * 10 + ctxL) * 10;
                        const int sp = ((const uint8_t *)W.src)[(4 * by + (px >> 2)) * 16 + 4 * bx + (px & 3)];
                        int best_rd = INTRA_INT_MAX, best_m = 0, best_d = 0;
                        for (int m0 = 0; m0 <= L.bmode_last; m0 += 4) {
                            const int m = min(m0 + (lane >> 4), 9);
                            const int t = sp - bpred_pixel(W.P, btab, m, px);
                            int d = t * t;
                            d += __shfl_xor(d, 8, 64); d += __shfl_xor(d, 4, 64); d += __shfl_xor(d, 2, 64); d += __shfl_xor(d, 1, 64);
                            const int rd = m0 + (lane >> 4) <= L.bmode_last ? rdcost(L.rdmult, L.rddiv, bc[m], d) : INTRA_INT_MAX;
#pragma unroll
                            for (int g = 0; g < 4; g++) {
                                const int rg = __builtin_amdgcn_readlane(rd, 16 * g), dg = __builtin_amdgcn_readlane(d, 16 * g);      // (scalars: the choice is the wave's)
                                if (rg < best_rd) { best_rd = rg; best_m = m0 + g; best_d = dg; }
                            }
                        }
                        // vp8_encode_intra4x4block
                        const int p = bpred_pixel(W.P, btab, best_m, px);
                        if (lane < 16) W.res[px] = (short)(sp - p);
                        compiler_fence();
                        if (lane == 0) {
                            int d[16], cf[16], q[16], dq[16], o[16];
#pragma unroll
                            for (int i = 0; i < 16; i++) d[i] = W.res[i];
                            quant_fdct(d, cf);
                            const int eob = L.fast ? quant_scan<true>(cf, tab, 0, q, dq) : quant_scan<false>(cf, tab, 0, q, dq);
                            if (eob > 1) {
                                int t[16];
#pragma unroll
                                for (int u = 0; u < 4; u++) {
                                    int v4[4];
                                    idct_col(dq[u], dq[4 + u], dq[8 + u], dq[12 + u], v4);
#pragma unroll
                                    for (int v = 0; v < 4; v++) t[4 * v + u] = (short)v4[v];
                                }
#pragma unroll
                                for (int v = 0; v < 4; v++) idct_row(t + 4 * v, o + 4 * v);
                            } else {
                                const int a1 = (dq[0] + 4) >> 3;     // vp8_dc_only_idct_add_c
#pragma unroll
                                for (int i = 0; i < 16; i++) o[i] = a1;
                            }
#pragma unroll
                            for (int i = 0; i < 16; i++) {
                                W.res[i] = (short)o[i];
                                W.blev[16 * b + i] = (short)(L.levels ? q[i] : dq[i]);
                            }
                            W.beob[b] = (uint8_t)eob;
                            W.bm[b] = (uint8_t)best_m;
                        }
                        compiler_fence();
                        if (lane < 16) W.fy[(4 * by + 1 + (px >> 2)) * FY_STRIDE + 4 + 4 * bx + (px & 3)] = (uint8_t)clamp255(p + W.res[px]);
                        compiler_fence();
                        cost += bc[best_m];
                        dist += best_d;
                        if (dist > best_sse) break;
                    }
                    if (b == 16) rd4 = rdcost(L.rdmult, L.rddiv, cost, dist);
                }

                // ---- 4. the decision; 5. the blocks of the 16x16 mode and of chroma
                const bool bpred = rd4 < rd16;
                if (bpred) best_rate = cost;
                int c16[16], q[16], dq[16];
                u32 pw[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                for (int i = 0; i < 16; i++) c16[i] = q[i] = dq[i] = 0;
                const bool luma = lane < 16, chroma = lane >= 16 && lane < 24;
                const int cpl = (lane >> 2) & 1, cbr = (lane >> 1) & 1, cbc = lane & 1;       // of a chroma lane: plane, block row, block column
                if ((luma && !bpred) || chroma) {
                    int d[16];
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        u32 sp;
                        if (luma) {
                            const int row = 4 * (lane >> 2) + i;
                            sp = W.src[4 * row + (lane & 3)];
                            pw[i] = intra_pred4(ymode, *(const u32 *)(W.fy + 4 + 4 * (lane & 3)), W.fy[(row + 1) * FY_STRIDE + 3], W.fy[3], dcy);
                        } else {
                            const int row = 4 * cbr + i;
                            const int dc = cpl ? dcs[1] : dcs[0];
                            sp = W.src[64 + 16 * cpl + 2 * row + cbc];
                            pw[i] = intra_pred4(uv_mode, *(const u32 *)(W.fc[cpl] + 4 + 4 * cbc), W.fc[cpl][(row + 1) * FC_STRIDE + 3], W.fc[cpl][3], dc);
                        }
#pragma unroll
                        for (int k = 0; k < 4; k++) d[4 * i + k] = (int)((sp >> (8 * k)) & 0xffu) - (int)((pw[i] >> (8 * k)) & 0xffu);
                    }
                    quant_fdct(d, c16);
                    if (luma) W.dcs[lane] = (short)c16[0];
                }
                compiler_fence();
                if (lane == 24 && !bpred) {
                    int d[16];
#pragma unroll
                    for (int i = 0; i < 16; i++) d[i] = W.dcs[i];
                    quant_walsh(d, c16);
                }
                int eob = 0;
                if (chroma || (lane < 25 && !bpred)) {
                    const int ty = lane < 16 ? 0 : lane < 24 ? 2 : 1;
                    eob = L.fast ? quant_scan<true>(c16, tab, ty, q, dq) : quant_scan<false>(c16, tab, ty, q, dq);
                } else if (luma)
                    eob = W.beob[lane];
                if (L.coef && lane < 25) {
                    u32x4_t w0, w1;
                    if (luma && bpred) {
                        w0 = *(const u32x4_t *)(W.blev + 16 * lane);
                        w1 = *(const u32x4_t *)(W.blev + 16 * lane + 8);
                    } else {
                        const int *o = L.levels ? q : dq;
#pragma unroll
                        for (int i = 0; i < 4; i++) {
                            w0[i] = (u32)(o[2 * i] & 0xffff) | (u32)o[2 * i + 1] << 16;
                            w1[i] = (u32)(o[8 + 2 * i] & 0xffff) | (u32)o[8 + 2 * i + 1] << 16;
                        }
                    }
                    GLOBAL_AS u32x4_t *cp = (GLOBAL_AS u32x4_t *)(coef + coef_stride * job + (size_t)mb * 800 + 32 * lane);
                    cp[0] = w0;
                    cp[1] = w1;
                }
                const u32 e4 = (u32)eob | (u32)__shfl_down(eob, 1, 64) << 8 | (u32)__shfl_down(eob, 2, 64) << 16 | (u32)__shfl_down(eob, 3, 64) << 24;
                if (L.eob && lane < 32 && (lane & 3) == 0) ((GLOBAL_AS u32 *)(eobs + eob_stride * job + (size_t)mb * 32))[lane >> 2] = e4;
                const bool coded = lane < 25 && (bpred ? (lane < 24 && eob != 0) : (lane < 16 ? eob >= 2 : eob != 0));
                const int skip = __builtin_amdgcn_ballot_w64(coded) == 0;        // mb_is_skippable
                const int eob_sum = wave_sum(eob);

                // the inverse side: the reconstruction is the neighbours' prediction, so it is always made
                if (lane == 24 && !bpred) {
                    int w[16];
                    if (eob > 1) quant_inv_walsh(dq, w);
                    else {
                        const int a1 = (short)((dq[0] + 3) >> 3);    // vp8_short_inv_walsh4x4_1_c
#pragma unroll
                        for (int i = 0; i < 16; i++) w[i] = a1;
                    }
#pragma unroll
                    for (int i = 0; i < 16; i++) W.dcs[i] = (short)w[i];
                }
                compiler_fence();
                if ((luma && !bpred) || chroma) {
                    const int dcf = luma ? 1 : tab[QT_DEQUANT + 4], acf = luma ? tab[QT_DEQUANT + 1] : tab[QT_DEQUANT + 5];
                    const int first = luma ? W.dcs[lane] : q[0];
                    int e = eob;
                    if (luma && e == 0 && first != 0) e = 1;         // eob_adjust
                    int rr[16];
                    if (e > 1) {
                        int in[16], t[16];
                        in[0] = (short)(first * dcf);
#pragma unroll
                        for (int i = 1; i < 16; i++) in[i] = (short)(q[i] * acf);
#pragma unroll
                        for (int u = 0; u < 4; u++) {
                            int o[4];
                            idct_col(in[u], in[4 + u], in[8 + u], in[12 + u], o);
#pragma unroll
                            for (int v = 0; v < 4; v++) t[4 * v + u] = (short)o[v];
                        }
#pragma unroll
                        for (int v = 0; v < 4; v++) idct_row(t + 4 * v, rr + 4 * v);
                    } else {
                        const int a1 = ((int)(short)(first * dcf) + 4) >> 3;
#pragma unroll
                        for (int i = 0; i < 16; i++) rr[i] = a1;
                    }
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const u32 o = add_clamp_pack(pw[i], rr + 4 * i);
                        if (luma) *(u32 *)(W.fy + (4 * (lane >> 2) + i + 1) * FY_STRIDE + 4 + 4 * (lane & 3)) = o;
                        else *(u32 *)(W.fc[cpl] + (4 * cbr + i + 1) * FC_STRIDE + 4 + 4 * cbc) = o;
                    }
                }
                if (lane < 16 && !bpred) W.bm[lane] = (uint8_t)(ymode == VP8IR_DC_PRED ? VP8IR_B_DC_PRED : ymode == VP8IR_V_PRED ? VP8IR_B_VE_PRED :
                                                                ymode == VP8IR_H_PRED ? VP8IR_B_HE_PRED : VP8IR_B_TM_PRED);
                compiler_fence();

                // ---- the lines for the neighbours, the outputs
                const u32 ry = *(const u32 *)(W.fy + ((lane >> 2) + 1) * FY_STRIDE + 4 + 4 * (lane & 3));
                const int crow = (lane & 15) >> 1, cg = lane & 1, cp2 = (lane >> 4) & 1;
                const u32 rc = *(const u32 *)(W.fc[cp2] + (crow + 1) * FC_STRIDE + 4 + 4 * cg);      // (read by lanes 0 .. 31)
                if (lane < INTRA_LINE_WORDS) {
                    u32 v;
                    if (lane < 4) v = *(const u32 *)(W.fy + 16 * FY_STRIDE + 4 + 4 * lane);
                    else if (lane < 8) v = *(const u32 *)(W.fc[(lane - 4) >> 1] + 8 * FC_STRIDE + 4 + 4 * (lane & 1));
                    else v = *(const u32 *)(W.bm + 12);
                    ring[rb][c & 3][lane] = v;
                    if (leave && rb == nr - 1) bound[c * INTRA_LINE_WORDS + lane] = v;
                } else if (lane >= 16 && lane < 32)
                    ((uint8_t *)rcol[rb])[lane - 16] = W.fy[(lane - 15) * FY_STRIDE + 19];
                else if (lane >= 32 && lane < 48) {
                    const int k = lane - 32;
                    ((uint8_t *)rcol[rb])[16 + k] = W.fc[k >> 3][((k & 7) + 1) * FC_STRIDE + 11];
                } else if (lane >= 48 && lane < 52)
                    ((uint8_t *)rcol[rb])[32 + lane - 48] = W.bm[4 * (lane - 48) + 3];
                if (L.modes && lane < 8) {
                    const u32 v = lane == 0 ? (u32)(bpred ? VP8IR_B_PRED : ymode) | (u32)uv_mode << 8 | (u32)skip << 16 :
                                  lane < 5 ? *(const u32 *)(W.bm + 4 * (lane - 1)) : 0u;
                    ((GLOBAL_AS u32 *)(modes + modes_stride * job + (size_t)mb * 32))[lane] = v;
                }
                if (L.planes) {
                    int recsse = 0;
                    if (L.planes & INTRA_RECSSE) {
                        int unused = 0;
                        recsse = sq_diff4(W.src[lane], ry, unused);
                        if (lane < 32) recsse += sq_diff4(W.src[64 + lane], rc, unused);
                        recsse = wave_sum(recsse);
                    }
                    if (lane == 0) {
                        GLOBAL_AS u32 *sp = (GLOBAL_AS u32 *)(stats + stats_stride * job) + mb;
                        if (L.planes & INTRA_RD16) { *sp = (u32)rd16; sp += nmb; }
                        if (L.planes & INTRA_RD4) { *sp = (u32)rd4; sp += nmb; }
                        if (L.planes & INTRA_RATE) { *sp = (u32)best_rate; sp += nmb; }
                        if (L.planes & INTRA_EOBS) { *sp = (u32)eob_sum; sp += nmb; }
                        if (L.planes & INTRA_RECSSE) *sp = (u32)recsse;
                    }
                }
                if (L.rec) {                                         // at the display size, the packed I420 layout: only what lies inside it
                    const int cw = (L.dw + 1) >> 1, ch = (L.dh + 1) >> 1;
                    GLOBAL_AS uint8_t *o = (GLOBAL_AS uint8_t *)(rec + rec_stride * job);
                    {
                        const int x = 16 * c + 4 * (lane & 3), y = 16 * r + (lane >> 2);
                        if (y < L.dh)
                            for (int i = 0; i < 4 && x + i < L.dw; i++) o[(size_t)y * L.dw + x + i] = (uint8_t)(ry >> (8 * i));
                    }
                    if (lane < 32) {
                        const int x = 8 * c + 4 * cg, y = 8 * r + crow;
                        const size_t base = (size_t)L.dw * L.dh + (cp2 ? (size_t)cw * ch : (size_t)0);
                        if (y < ch)
                            for (int i = 0; i < 4 && x + i < cw; i++) o[base + (size_t)y * cw + x + i] = (uint8_t)(rc >> (8 * i));
                    }
                }
                compiler_fence();
            }
            __syncthreads();
        }
    }
}
