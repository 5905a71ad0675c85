// The decoder's debug overlays (vp8/common/postproc.c:1007-1362, CONFIG_POSTPROC_VISUALIZER) for gfx950, drawn in place into one
// frame buffer's raster form, in the reference's order -- later phases overwrite or blend over earlier ones:
//   1. text (vp8_blit_text): the frame-info string, a character per macroblock (its mode, or its "DC diff" digit), the rate string;
//      each character a 7x5 cell of 0 / 255, addressed linearly from the luma origin with the luma stride
//   2. motion vectors (vp8_blit_line): Bresenham lines whose pixels are inverted -- a lane per line, the pixels combined with
//      32-bit atomic XORs on the word holding the byte: XOR commutes, so the result does not depend on the order
//   3. block-mode colours (vp8_blend_mb_inner / vp8_blend_b) and 4. reference-frame colours (vp8_blend_mb_outer): alpha blends,
//      a lane per pixel that applies both in order
// Every write is bounds-checked against the frame buffer: a line or a string that leaves the picture lands in the border or in
// the next plane as in the reference, never outside the buffer.  vp8hip_visualize (vp8hip_visualize.hip) launches them.
//
// The glyphs and colours are the reference's numbers as tests/golden/vis_tables.json recorded them from a visualizer build
// (tests/test_visualizer_cpu.py compares the tables below with that record).
#include "vp8_common.hip.h"
#include "vp8_ir.h"

namespace {

enum { TXT_FRAME_INFO = 1 << 3, TXT_MBLK_MODES = 1 << 4, TXT_DC_DIFF = 1 << 5, TXT_RATE_INFO = 1 << 6,
       DRAW_MV = 1 << 7, CLR_BLK_MODES = 1 << 8, CLR_FRM_REF_BLKS = 1 << 9 };

// bit r * 7 + c: row r (0..4), column c (0..6) of the character's cell is 255, else 0; characters outside 0..127 are blank
__constant__ unsigned long long vis_glyph[128] = {
    0x0ull, 0x0ull, 0x0ull, 0x0ull, 0x0ull, 0x0ull, 0x0ull, 0x0ull,
    0x0ull, 0x0ull, 0x0ull, 0x0ull, 0x0ull, 0x0ull, 0x0ull, 0x0ull,
    0x0ull, 0x0ull, 0x0ull, 0x0ull, 0x0ull, 0x0ull, 0x0ull, 0x0ull,
    0x0ull, 0x0ull, 0x0ull, 0x0ull, 0x0ull, 0x0ull, 0x0ull, 0x0ull,
    0x0ull, 0x40010204ull, 0xaull, 0xa3e28f8aull, 0xe1818704ull, 0x110410411ull, 0x163410504ull, 0x408ull,
    0x40408104ull, 0x41020404ull, 0x1410500ull, 0x838200ull, 0xc1000000ull, 0x38000ull, 0x80000000ull, 0x10410410ull,
    0xe2654c8eull, 0xe0810304ull, 0x1f043088eull, 0xe223088eull, 0x8107c50cull, 0x7101c08full, 0x61218086ull, 0x8102089full,
    0xe223888eull, 0xe203888eull, 0x800200ull, 0x20800200ull, 0x80808208ull, 0x1c00700ull, 0x20820202ull, 0x40010486ull,
    0xe027488eull, 0x113e4488eull, 0xf223c88full, 0xe020408eull, 0xf224488full, 0x1f021c09full, 0x1021c09full, 0xe226408eull,
    0x11227c891ull, 0x1f081021full, 0xe224081eull, 0x90a0c289ull, 0x1f0204081ull, 0x112254d91ull, 0x113254991ull, 0xe224488eull,
    0x1023c88full, 0x16124488eull, 0x11123c88full, 0xe203808eull, 0x4081021full, 0x1f2244891ull, 0x41444891ull, 0xa2a44891ull,
    0x111410511ull, 0x40810511ull, 0x1f041041full, 0x0ull, 0x0ull, 0x0ull, 0x0ull, 0x0ull,
    0x0ull, 0x113e4488eull, 0xf223c88full, 0xe020408eull, 0xf224488full, 0x1f021c09full, 0x1021c09full, 0xe226408eull,
    0x11227c891ull, 0x1f081021full, 0xe224081eull, 0x90a0c289ull, 0x1f0204081ull, 0x112254d91ull, 0x113254991ull, 0xe224488eull,
    0x1023c88full, 0x16124488eull, 0x11123c88full, 0xe203808eull, 0x4081021full, 0x1f2244891ull, 0x41444891ull, 0xa2a44891ull,
    0x111410511ull, 0x40810511ull, 0x1f041041full, 0x0ull, 0x0ull, 0x0ull, 0x0ull, 0x0ull,
};
// Y, U, V per macroblock mode (DC_PRED .. SPLITMV), per sub-block mode (B_DC_PRED .. B_HU_PRED), per reference frame
__constant__ uint8_t vis_mb_colour[10][3] = {
    {196, 99, 91}, {144, 53, 34}, {193, 48, 106}, {98, 97, 89}, {66, 98, 91}, {203, 146, 86}, {147, 153, 99}, {29, 189, 118},
    {64, 168, 145}, {81, 90, 239}};
__constant__ uint8_t vis_b_colour[10][3] = {
    {92, 210, 135}, {119, 194, 180}, {127, 164, 206}, {117, 120, 213}, {105, 202, 94}, {100, 200, 214}, {45, 201, 135},
    {137, 82, 198}, {156, 173, 57}, {144, 54, 120}};
__constant__ uint8_t vis_ref_colour[4][3] = {{144, 53, 34}, {40, 239, 109}, {210, 16, 146}, {81, 90, 239}};

// Text.  mode 0: the string str[0..len) at the luma origin; 1: per macroblock its mode + 'a'; 2: per macroblock 'a' (key frame)
// or its DC-diff digit.  A lane per cell pixel (35 per character).  A string longer than a row wraps onto the rows below, where a
// later character's upper rows cover an earlier one's lower rows: the reference writes character after character, so of the
// pixels several lanes address the lane of the latest character writes (its row r - 1 lies stride bytes further on: the cell a
// row further down belongs to a later character exactly when k + stride is still inside the string).
__global__ __launch_bounds__(256) void vp8_vis_text_kernel(uint8_t *__restrict__ fb, int frame_size, DevGeom g,
                                                           const vp8ir_mbx *__restrict__ mbx, const char *__restrict__ str, int len,
                                                           int mode, int key_frame)
{
    const int units = mode == 0 ? len : g.mb_cols * g.mb_rows;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= units * 35) return;
    const int u = t / 35, cell = t % 35, r = cell / 7, c = cell % 7;
    int ch;
    long p;
    if (mode == 0) {
        const int k = 7 * u + c;
        if (r > 0 && k + g.y_stride < 7 * len) return;          // a later character writes this byte after us
        ch = (unsigned char)str[u];
        p = (long)g.y_off + k + (long)r * g.y_stride;
    } else {
        const vp8ir_mb &m = mbx[u].d;
        if (mode == 1) ch = m.y_mode + 'a';
        else if (key_frame) ch = 'a';
        else ch = (m.y_mode != VP8IR_B_PRED && m.y_mode != VP8IR_SPLITMV && (m.flags & VP8IR_MB_SKIP)) ? '0' : '1';
        const int row = u / g.mb_cols, col = u % g.mb_cols;
        p = (long)g.y_off + (long)(16 * row + 4 + r) * g.y_stride + 16 * col + 4 + c;
    }
    const unsigned long long bits = ch < 128 ? vis_glyph[ch] : 0ull;
    if (p >= 0 && p < frame_size) fb[p] = ((bits >> (r * 7 + c)) & 1) ? 255 : 0;
}

__device__ __forceinline__ void plot(uint8_t *fb, int frame_size, const DevGeom &g, int x, int y)
{
    const long p = (long)g.y_off + x + (long)y * g.y_stride;
    if (p < 0 || p >= frame_size) return;
    unsigned int *w = (unsigned int *)(fb + (p & ~3l));
    atomicXor(w, 255u << (8 * (int)(p & 3)));
}

// vp8_blit_line: Bresenham, one point per step along the longer axis, both ends included
__device__ void blit_line(uint8_t *fb, int frame_size, const DevGeom &g, int x0, int x1, int y0, int y1)
{
    const bool steep = abs(y1 - y0) > abs(x1 - x0);
    int t;
    if (steep) { t = x0; x0 = y0; y0 = t; t = x1; x1 = y1; y1 = t; }
    if (x0 > x1) { t = x0; x0 = x1; x1 = t; t = y0; y0 = y1; y1 = t; }
    const int dx = x1 - x0, dy = abs(y1 - y0), ystep = y0 < y1 ? 1 : -1;
    int err = dx / 2, y = y0;
    for (int x = x0; x <= x1; x++) {
        if (steep) plot(fb, frame_size, g, y, x);
        else plot(fb, frame_size, g, x, y);
        err -= dy;
        if (err < 0) { y += ystep; err += dx; }
    }
}

// constrain_line (postproc.c:652-694): the far end clipped to 0..width, 0..height (inclusive), one side after the other
__device__ void constrain_line(int x0, int *x1, int y0, int *y1, int width, int height)
{
    int dx, dy;
    if (*x1 > width) { dx = *x1 - x0; dy = *y1 - y0; *x1 = width; if (dx) *y1 = ((width - x0) * dy) / dx + y0; }
    if (*x1 < 0) { dx = *x1 - x0; dy = *y1 - y0; *x1 = 0; if (dx) *y1 = ((0 - x0) * dy) / dx + y0; }
    if (*y1 > height) { dx = *x1 - x0; dy = *y1 - y0; *y1 = height; if (dy) *x1 = ((height - y0) * dx) / dy + x0; }
    if (*y1 < 0) { dx = *x1 - x0; dy = *y1 - y0; *y1 = 0; if (dy) *x1 = ((0 - y0) * dx) / dy + x0; }
}

// Motion vectors (postproc.c:1095-1254): lane (macroblock, line) -- line k < 16 of a 4x4 split, k < 4 / 2 of the other
// partitionings, k == 0 the 16x16 vector (both of its lines: the second is clipped from where the first left the far end).
// The 16x8, 8x16 and 8x8 partitionings draw every line with block 0's vector, as the reference does.  Inter frames only.
__global__ __launch_bounds__(256) void vp8_vis_mv_kernel(uint8_t *__restrict__ fb, int frame_size, DevGeom g,
                                                         const vp8ir_mbx *__restrict__ mbx, const vp8ir_mv *__restrict__ mvs, int mask)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int nmb = g.mb_cols * g.mb_rows;
    if (t >= nmb * 16) return;
    const int mb = t >> 4, k = t & 15;
    const vp8ir_mb &m = mbx[mb].d;
    const int mode = m.y_mode;
    if (mode > VP8IR_SPLITMV || !(mask & (1 << mode)) || mode < VP8IR_NEARESTMV) return;
    const int x0 = 16 * (mb % g.mb_cols), y0 = 16 * (mb / g.mb_cols);
    const int W = g.aligned_w, H = g.aligned_h;
    int sx, sy, x1, y1;
    if (mode == VP8IR_SPLITMV) {
        const int part = m.partitioning;
        vp8ir_mv mv;
        if (part == 0) {
            if (k >= 2) return;
            sx = x0 + 8; sy = y0 + 4 + 8 * k; mv = mvs[mb * 16];
        } else if (part == 1) {
            if (k >= 2) return;
            sx = x0 + 4 + 8 * k; sy = y0 + 8; mv = mvs[mb * 16];
        } else if (part == 2) {
            if (k >= 4) return;
            sx = x0 + 4 + 8 * (k & 1); sy = y0 + 4 + 8 * (k >> 1); mv = mvs[mb * 16];
        } else {
            sx = x0 + 4 * (k & 3) + 2; sy = y0 + 4 * (k >> 2) + 2; mv = mvs[mb * 16 + k];
        }
        x1 = sx + (mv.col >> 3);
        y1 = sy + (mv.row >> 3);
        constrain_line(sx, &x1, sy, &y1, W, H);
        blit_line(fb, frame_size, g, sx, x1, sy, y1);
        return;
    }
    if (k) return;
    const vp8ir_mv mv = mvs[mb * 16];
    const int lx0 = x0 + 8, ly0 = y0 + 8;
    x1 = lx0 + (mv.col >> 3);
    y1 = ly0 + (mv.row >> 3);
    if (x1 != lx0 && y1 != ly0) {
        constrain_line(lx0, &x1, ly0 - 1, &y1, W, H);
        blit_line(fb, frame_size, g, lx0, x1, ly0 - 1, y1);
        constrain_line(lx0, &x1, ly0 + 1, &y1, W, H);
        blit_line(fb, frame_size, g, lx0, x1, ly0 + 1, y1);
    } else
        blit_line(fb, frame_size, g, lx0, x1, ly0, y1);
}

__device__ __forceinline__ uint8_t blend(int v, int colour) { return (uint8_t)((v * 0xc000 + colour * 0x4000) >> 16); }

// Colours (postproc.c:1257-1360): a lane per pixel of the coded area, luma then U then V.  Block modes: B_PRED macroblocks take
// each sub-block's colour over the whole sub-block when the mb-modes mask has the VALUE 4 or the b-modes mask has bit B_PRED
// (the reference tests `display_mb_modes_flag & B_PRED`); other macroblocks whose mode is in the mb-modes mask their mode's colour
// inside a 2-pixel (chroma: 1) margin.  Then the reference-frame colour on that margin, for reference frames in its mask.
__global__ __launch_bounds__(256) void vp8_vis_colour_kernel(uint8_t *__restrict__ fb, DevGeom g, const vp8ir_mbx *__restrict__ mbx,
                                                             int blk_modes, int mb_mask, int b_mask, int ref_mask)
{
    const int W = g.aligned_w, H = g.aligned_h;
    const long luma = (long)W * H, chroma = (long)(W / 2) * (H / 2);
    long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= luma + 2 * chroma) return;
    int plane = 0, w = W, n = 16;
    if (t >= luma) { t -= luma; plane = 1 + (int)(t / chroma); t %= chroma; w = W / 2; n = 8; }
    const int x = (int)(t % w), y = (int)(t / w);
    const int lx = x % n, ly = y % n, last = n - 1;
    const vp8ir_mb &m = mbx[(y / n) * g.mb_cols + x / n].d;
    uint8_t *p = fb + (plane == 0 ? (long)g.y_off + (long)y * g.y_stride
                                  : (long)(plane == 1 ? g.u_off : g.v_off) + (long)y * g.uv_stride) + x;
    int v = *p;
    const int v0 = v;
    const int mode = m.y_mode < 10 ? m.y_mode : 0;
    if (blk_modes) {
        if (mode == VP8IR_B_PRED && ((mb_mask & VP8IR_B_PRED) || b_mask)) {
            if ((b_mask & (1 << mode)) || (mb_mask & VP8IR_B_PRED)) {
                const int blk = plane == 0 ? (ly >> 2) * 4 + (lx >> 2) : (ly >> 1) * 4 + (lx >> 1);
                const int bm = m.b_modes[blk] < 10 ? m.b_modes[blk] : 0;
                v = blend(v, vis_b_colour[bm][plane]);
            }
        } else if ((mb_mask & (1 << mode)) && lx >= n / 8 && lx < n - n / 8 && ly >= n / 8 && ly < n - n / 8)
            v = blend(v, vis_mb_colour[mode][plane]);
    }
    const int rf = m.ref_frame & 3;
    if (ref_mask & (1 << rf)) {
        const int e = n / 8;                 // margin: 2 luma, 1 chroma
        if (lx < e || lx > last - e || ly < e || ly > last - e) v = blend(v, vis_ref_colour[rf][plane]);
    }
    if (v != v0) *p = (uint8_t)v;
}

}  // namespace

// launch wrappers used by vp8hip_visualize (vp8hip_visualize.hip)
void vp8vis_text(hipStream_t st, uint8_t *fb, int frame_size, const DevGeom &g, const vp8ir_mbx *mbx, const char *str, int len,
                 int mode, int key_frame)
{
    const long lanes = 35l * (mode == 0 ? len : g.mb_cols * g.mb_rows);
    if (lanes <= 0) return;
    hipLaunchKernelGGL(vp8_vis_text_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, fb, frame_size, g, mbx, str,
                       len, mode, key_frame);
}
void vp8vis_mvs(hipStream_t st, uint8_t *fb, int frame_size, const DevGeom &g, const vp8ir_mbx *mbx, const vp8ir_mv *mvs, int mask)
{
    const long lanes = 16l * g.mb_cols * g.mb_rows;
    hipLaunchKernelGGL(vp8_vis_mv_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, fb, frame_size, g, mbx, mvs, mask);
}
void vp8vis_colours(hipStream_t st, uint8_t *fb, const DevGeom &g, const vp8ir_mbx *mbx, int blk_modes, int mb_mask, int b_mask,
                    int ref_mask)
{
    const long lanes = (long)g.aligned_w * g.aligned_h * 3 / 2;
    hipLaunchKernelGGL(vp8_vis_colour_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, fb, g, mbx, blk_modes, mb_mask,
                       b_mask, ref_mask);
}
