// The transform coefficients of IR slots as tensors in device memory (vp8hip_frames_coef_async, vp8hip_coef.hip; include/vp8hip.h has
// the definition): the levels the stream codes, or the `short`s that enter the inverse transforms, made from the slots as they lie in
// HBM (include/vp8_ir.h: vp8ir_mbx records, the block stream through d.sparse_first).  vp8_residual.hip's shape without its inverse DCT.
//
// A workgroup takes a run of up to COEF_RUN macroblocks of one macroblock row.
//   1. stage   the run's records, 128 bytes each, into LDS with 16-byte loads
//   2. a lane per macroblock   keeps the Y2 block as the record has it, then res_macroblock (vp8_res_mb.hip.h): the segment's six
//      factors, the mask of blocks that have 32 bytes in the stream, and the Y2 block's inverse WHT, whose sixteen DCs replace y2[] in
//      the staged record.  The lane then writes the Y2 plane of its macroblock into the image.
//   3. a lane per block   its 32 bytes at sparse_first + popcount(mask below k), two 16-byte loads, or its lone first coefficient from
//      the record, or nothing; dequantised or not; sixteen int16 into the run's image in LDS.
//   4. output  a lane makes four neighbouring elements of a plane's row from the image and stores them as one piece, neighbouring
//      lanes contiguous (the walk, tensor_value and tensor_store4 of vp8_tensor_out.hip.h).
// The image is arranged as the tensor is, so that phase 4 reads rows: a plane of cells G x G a macroblock (Y 4, U and V 2, Y2 1) is
//   CHANNELS  [16 * G rows: channel j, block row br at j * G + br][G * COEF_RUN block columns + 8]      channels >= nfreq: not written
//   INPLACE   [4 * G rows][4 * G * COEF_RUN columns + 8]: vp8_residual.hip's image
// in int16.  The 16 bytes of padding a row put the block rows of a macroblock, which the lanes of its blocks write at once, on
// different banks: a CHANNELS row of Y is 272 bytes, 4 banks (of the 32 a store goes by) on from the row above, so that the sixteen
// luma lanes of a macroblock, two to a dword, fall on eight banks and the next macroblock's on the eight beside them.
// Integer and conversion arithmetic only.
#include "vp8_res_mb.hip.h"
#include "vp8_tensor_out.hip.h"

#define COEF_REC_WORDS (COEF_RUN * VP8IR_MBX_WORDS)
#define COEF_PAD 8
// the image's planes one behind the other, in shorts: the CHANNELS form, the larger (INPLACE: 400 a macroblock and 28 rows)
#define COEF_IMG (400 * COEF_RUN + (16 * 4 + 2 * 16 * 2 + 16) * COEF_PAD)

struct CoefPlane {
    short *img;                                  // the plane's image in LDS, row stride `stride` shorts
    int stride;
    int G;                                       // cells of a macroblock each way: 4, 2, 2, 1
};

// the planes of the image: G, the rows and the row stride by layout
__device__ __forceinline__ void coef_planes(short *img, int layout, CoefPlane (&pl)[COEF_PLANES])
{
    int at = 0;
#pragma unroll
    for (int p = 0; p < COEF_PLANES; p++) {
        const int G = p == 0 ? 4 : p == 3 ? 1 : 2;
        const int rows = layout == COEF_INPLACE ? 4 * G : 16 * G;
        const int stride = (layout == COEF_INPLACE ? 4 * G : G) * COEF_RUN + COEF_PAD;
        pl[p].img = img + at;
        pl[p].stride = stride;
        pl[p].G = G;
        at += rows * stride;
    }
}

// the sixteen values v[] of a block, indexed as the IR stores them (v[u * 4 + v] is position (v, u)), into the image of its plane:
// block (br, bc) of macroblock number mb of the run
__device__ __forceinline__ void coef_put(const int (&v)[16], const CoefPlane &pl, int mb, int br, int bc, const CoefLaunch &L)
{
    if (L.layout == COEF_INPLACE) {
        short *o = pl.img + (br * 4) * pl.stride + (mb * pl.G + bc) * 4;
#pragma unroll
        for (int r = 0; r < 4; r++)              // row r: positions (r, 0..3) = v[r], v[4 + r], v[8 + r], v[12 + r]
            *(u32x2 *)(o + r * pl.stride) = u32x2{ ((u32)v[r] & 0xffffu) | ((u32)v[4 + r] << 16), ((u32)v[8 + r] & 0xffffu) | ((u32)v[12 + r] << 16) };
        return;
    }
    short *o = pl.img + br * pl.stride + mb * pl.G + bc;
    const int step = pl.G * pl.stride;           // a channel on
    const bool zz = L.zigzag != 0;
#pragma unroll
    for (int j = 0; j < 16; j++) {
        if (j >= L.nfreq) break;
        // channel j is position j = 4v + u, or the VP8 scan's (vp8_default_zig_zag1d); the IR holds it at u * 4 + v
        constexpr int scan[16] = { 0, 1, 4, 8, 5, 2, 3, 6, 9, 12, 13, 10, 7, 11, 14, 15 };
        const int pr = (j & 3) * 4 + (j >> 2), pz = (scan[j] & 3) * 4 + (scan[j] >> 2);
        o[j * step] = (short)(zz ? v[pz] : v[pr]);
    }
}

// phase 2, a lane per macroblock: number mb of the run, staged at rec
__device__ __forceinline__ void coef_macroblock(unsigned *rec, int mb, const ResSlot &hs, const CoefPlane &py2, const CoefLaunch &L)
{
    int v[16];
    {
        const u32x4 *y2 = (const u32x4 *)(rec + 16);
        const u32x4 a = y2[0], b = y2[1];
        const u32 q[8] = { a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w };
#pragma unroll
        for (int i = 0; i < 16; i++) v[i] = (i & 1) ? hi16(q[i >> 1]) : sext16(q[i >> 1]);
    }
    res_macroblock(rec, hs);
    if (!(L.planes & VP8HIP_COEF_Y2)) return;
    const u32 r0 = rec[0];
    const u32 y_mode = r0 & 255u;
    const bool skip = (r0 >> 24) & VP8IR_MB_SKIP;
    const bool has_y2 = y_mode != VP8IR_B_PRED && y_mode != VP8IR_SPLITMV;
    const int eob = ((const unsigned char *)rec)[8 + 24];
    const u32 dq = rec[RES_W_DQ + 1];
    const bool levels = L.stage == COEF_LEVELS;
    const int dc = levels ? 1 : (int)(dq & 0xffffu), ac = levels ? 1 : (int)(dq >> 16);
    const bool none = !has_y2 || skip || eob == 0;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const int keep = none || (i && eob == 1) ? 0 : v[i];
        v[i] = (short)(keep * (i ? ac : dc));    // vp8_dequantize_b_c
    }
    coef_put(v, py2, mb, 0, 0, L);
}

// phase 3, a lane per block: block k of the macroblock staged at rec, which is number mb of the run
__device__ __forceinline__ void coef_block(const unsigned *rec, int mb, int k, const char *__restrict__ blocks, unsigned cap_blocks, const CoefPlane (&pl)[COEF_PLANES],
                                           const CoefLaunch &L)
{
    const u32 r0 = rec[0];
    const u32 y_mode = r0 & 255u;
    const bool skip = (r0 >> 24) & VP8IR_MB_SKIP;
    const bool has_y2 = y_mode != VP8IR_B_PRED && y_mode != VP8IR_SPLITMV;
    const bool luma = k < 16;
    const bool dc_given = luma && has_y2;        // its DC is not coded here: the Y2 block has it
    const u32 dq = rec[RES_W_DQ + (luma ? 0 : 2)];
    const int first = ((const short *)(rec + 16))[k];          // y2[16] and cdc[8] lie one behind the other; dc_given: the WHT's DC by now
    const int eob = ((const unsigned char *)rec)[8 + k];
    const u32 mask = rec[RES_W_MASK];
    int v[16];
    if ((mask >> k) & 1u) {
        const GLOBAL_AS u32x4 *p = res_block_at(rec, mask, k, blocks, cap_blocks);
        const u32x4 ca = p[0], cb = p[1];
        const u32 q[8] = { ca.x, ca.y, ca.z, ca.w, cb.x, cb.y, cb.z, cb.w };
#pragma unroll
        for (int i = 0; i < 16; i++) v[i] = (i & 1) ? hi16(q[i >> 1]) : sext16(q[i >> 1]);
    } else {
#pragma unroll
        for (int i = 1; i < 16; i++) v[i] = 0;
        v[0] = !skip && eob == 1 ? first : 0;    // vp8ir_block_kind 1 (dc_given: below)
    }
    if (dc_given) v[0] = 0;
    if (L.stage == COEF_DEQUANT) {
        const int dqdc = (int)(dq & 0xffffu), dqac = (int)(dq >> 16);
#pragma unroll
        for (int i = 0; i < 16; i++) v[i] = (short)(v[i] * (i ? dqac : dqdc));         // vp8_dequantize_b_c
        if (dc_given && !skip) v[0] = first;     // factor 1 (decodframe.c:92)
    }
    if (luma) coef_put(v, pl[0], mb, k >> 2, k & 3, L);
    else coef_put(v, pl[k >= 20 ? 2 : 1], mb, ((k - 16) & 3) >> 1, k & 1, L);
}

// phase 4 for one plane: `nrows` rows of the image, columns 0 .. w - 1 of each, to the tensor's plane at dst, W elements a row: image
// row r is the plane's row (r >> lg) * chan + base + (r & ((1 << lg) - 1)), its column 0 the plane's column xa (a multiple of 4)
template <int DTYPE>
__device__ __forceinline__ void coef_emit(const CoefPlane &pl, int nrows, int lg, size_t chan, int base, int xa, int w, int W, uint8_t *dst, float scale,
                                          bool vec)
{
    typedef typename TensorElem<DTYPE>::T elem_t;
    constexpr int ES = (int)sizeof(elem_t);
    TensorWalk t((w + 3) >> 2);                  // over the groups of four the columns touch
#pragma unroll 1
    for (; t.row < nrows; t.next()) {
        const int r = t.row, x = t.col << 2;
        const u32x2 d = *(const u32x2 *)(pl.img + r * pl.stride + x);     // (a group the run's end cuts: the row's padding behind it)
        const int v[4] = { sext16(d.x), hi16(d.x), sext16(d.y), hi16(d.y) };
        unsigned e[4];
        tensor_values4<DTYPE>(v, scale, e);
        const size_t row = (size_t)(r >> lg) * chan + (size_t)(base + (r & ((1 << lg) - 1)));
        uint8_t *o = dst + (row * (size_t)W + (size_t)(xa + x)) * ES;
        if (vec && x + 4 <= w) tensor_store4<ES>(o, e);
        else {
#pragma unroll
            for (int i = 0; i < 4; i++)
                if (x + i < w) ((GLOBAL_AS elem_t *)o)[i] = (elem_t)e[i];
        }
    }
}

template <int DTYPE>
__device__ __forceinline__ void coef_body(const char *__restrict__ slot_base, size_t slot_bytes, size_t o_mbx, size_t o_blocks, const char *__restrict__ pool,
                                          unsigned cap_blocks, uint8_t *__restrict__ dst, size_t dst_stride, const CoefLaunch &L)
{
    constexpr int ES = (int)sizeof(typename TensorElem<DTYPE>::T);
    __shared__ __attribute__((aligned(16))) unsigned lrec[COEF_REC_WORDS];
    __shared__ __attribute__((aligned(16))) short img[COEF_IMG];
    const int f = (int)blockIdx.y;
    const int cols = L.mb_cols;
    const int m = (int)blockIdx.x / L.runs, c0 = ((int)blockIdx.x - m * L.runs) * COEF_RUN, c1 = min(c0 + COEF_RUN, cols), nmbs = c1 - c0;
    CoefPlane pl[COEF_PLANES];
    coef_planes(img, L.layout, pl);

    const ResSlot hs = L.s[f];
    const char *slot = slot_base + slot_bytes * (size_t)hs.slot;
    {
        const GLOBAL_AS u32x4 *grec = (const GLOBAL_AS u32x4 *)(slot + o_mbx) + ((size_t)m * cols + c0) * 8;
        if ((int)threadIdx.x < nmbs * 8) ((u32x4 *)lrec)[threadIdx.x] = grec[threadIdx.x];
    }
    __syncthreads();
    if ((int)threadIdx.x < nmbs) coef_macroblock(lrec + threadIdx.x * VP8IR_MBX_WORDS, (int)threadIdx.x, hs, pl[3], L);
    __syncthreads();
    {
        const char *blocks = pool ? pool : slot + o_blocks;
#pragma unroll 1
        for (int b = threadIdx.x; b < nmbs * 24; b += 256) {
            const int mb = b / 24, k = b - mb * 24;
            if ((L.planes >> (k < 16 ? 0 : k < 20 ? 1 : 2)) & 1u) coef_block(lrec + mb * VP8IR_MBX_WORDS, mb, k, blocks, cap_blocks, pl, L);
        }
    }
    __syncthreads();

    uint8_t *D = dst + dst_stride * f;
    const bool inplace = L.layout == COEF_INPLACE;
#pragma unroll
    for (int p = 0; p < COEF_PLANES; p++) {
        if (!((L.planes >> p) & 1u)) continue;
        const int G = pl[p].G, lgG = p == 0 ? 2 : p == 3 ? 0 : 1;
        const int cell = inplace ? 4 * G : G;    // columns and rows of a macroblock in a channel (INPLACE: in the plane)
        uint8_t *o = D + (size_t)L.off[p] * ES;
        const bool vec = (L.vec >> p) & 1u;
        // CHANNELS: channel j's G rows of this macroblock row; INPLACE: the plane's 4G rows of it, as one channel
        coef_emit<DTYPE>(pl[p], inplace ? cell : L.nfreq * G, inplace ? lgG + 2 : lgG, inplace ? 0 : (size_t)G * L.mb_rows, cell * m, cell * c0, cell * nmbs,
                         cell * cols, o, L.scale[p], vec);
    }
}

// grid: x = the runs of a frame (mb_rows * L.runs), y = the frames of the launch.  slot_base: IR slot 0, slot_bytes apart, records at
// o_mbx and the block stream at o_blocks inside -- or, with pool not null, every slot's blocks in the pool, counted from its start;
// cap_blocks: blocks either holds.  dst: the launch's first frame.
#define COEF_KERNEL(NAME, DTYPE)                                                                                                             \
    extern "C" __global__ void __launch_bounds__(256)                                                                                        \
    NAME(const char *__restrict__ slot_base, size_t slot_bytes, size_t o_mbx, size_t o_blocks, const char *__restrict__ pool, unsigned cap_blocks, \
         uint8_t *__restrict__ dst, size_t dst_stride, CoefLaunch L)                                                                         \
    {                                                                                                                                        \
        coef_body<DTYPE>(slot_base, slot_bytes, o_mbx, o_blocks, pool, cap_blocks, dst, dst_stride, L);                                      \
    }
COEF_KERNEL(vp8_coef_i16_kernel, TENSOR_I16)
COEF_KERNEL(vp8_coef_f16_kernel, TENSOR_F16)
COEF_KERNEL(vp8_coef_f32_kernel, TENSOR_F32)
