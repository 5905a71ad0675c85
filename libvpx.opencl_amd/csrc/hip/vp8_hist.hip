// Byte histograms (vp8hip_frames_hist_async, vp8hip_slots_hist_async, vp8hip_trace_wear_hist_async, vp8hip_trace_cover_hist_async;
// vp8hip_hist.hip has the plans, include/vp8hip.h the definitions): 256 uint32 counts per plane of a U8 tensor another call of the
// family would hand out -- a picture's planes or the absolute difference of two pictures', a slot's info planes on the native grid,
// the planes of a wear or a COUNT entry -- without that tensor ever existing.  The library's one reducing kernel family.
//
// ONE BODY.  A workgroup of four waves keeps 4 * LREP private sub-histograms per plane in LDS, HIST_ROW dwords apart: a lane adds
// to the copy of its wave and of its lane number modulo LREP with an LDS atomic without return (ds_add_u32).  Two things keep a flat
// plane, which sends every lane to one bin, from serialising a wave on one LDS address: the LREP copies, and the merge of equal
// neighbours among a lane's values before the add (hist_add4, hist_add_dword, hist_add16: four equal values are one add of 4, and
// sixteen equal bytes of a picture ONE add of 16 where noise costs sixteen adds of 1).  The merge is by whole groups and no finer:
// DESIGN 4.20 has what a run-by-run merge cost in instructions.  HIST_ROW = 257 puts the same bin of neighbouring copies into
// neighbouring banks.  After a barrier, lane t sums bin t & 255 of plane t >> 8 over the copies and writes it out: with a plain
// store where the workgroup owns the job's output (gridDim.x == 1), else -- vp8_hist_fill_kernel has zeroed the outputs on the same
// stream -- with a global integer atomic add without return, one per non-zero bin.  Integer adds commute: the same bits in every
// run, whatever order lanes and workgroups arrive in.
//
// FOUR SOURCES.
//   pictures   a lane takes sixteen neighbouring columns of a row of one plane, Y, U, V one after the other through the same LDS:
//              from the raster form one 16-byte load (rows of every plane start on 16-byte boundaries and end in a border wider than
//              the piece), from the tiles four aligned dwords (hist_read16, vp8_frame_read.hip.h; ScaleSrc<SCALE_FROM_TILES>::atN<4>, vp8_scale_src.hip.h: the one
//              place that knows the tiles); a frame buffer never written reads as zeros and no address is formed.  The two frames
//              of a pair are read independently, each in its form.  Columns past the plane's width are loaded where the aligned
//              area has them and never counted.
//   slots      staged as vp8_side.hip stages them (side_stage, vp8_side_src.hip.h: records and, for MVMAG on an inter frame, vectors
//              of a group of macroblock rows with 16-byte loads); a lane takes the four cells of one row of a macroblock's blocks
//              through side_cell, the one place that says what the planes are.
//   entries    pool entries are d_w * d_h dwords in a row: a lane takes four neighbours with one 16-byte load aligned to a dword
//              (load4_dword_aligned, vp8_trace_read.hip.h), the tail dword by dword, and WearPlanes / CoverPlanes say what a dword's
//              planes are.  Pool values are data and never addresses.
// Workgroups share a job by rows (tensor_share), as the invert's do.  Nothing but the outputs is written.
#include "vp8_frame_read.hip.h"
#include "vp8_side_src.hip.h"
#include "vp8_trace_read.hip.h"
#include "vp8hip.h"

typedef __attribute__((address_space(3))) unsigned *lds_u32p;

// the sub-histograms of a workgroup: plane p's copy k at (p * C + k) * HIST_ROW
template <int LREP>
struct HistLds {
    static constexpr int C = 4 * LREP;
    unsigned *lds;
    int copy;                                    // this lane's: its wave's LREP copies, by lane number
    __device__ __forceinline__ HistLds(unsigned *lds_) : lds(lds_), copy((int)(threadIdx.x >> 6) * LREP + (int)(threadIdx.x & (LREP - 1))) {}
    __device__ __forceinline__ unsigned *plane(int p) const { return lds + (p * C + copy) * HIST_ROW; }

    // zero np planes; barriers on both sides: whatever read or staged LDS before is done, and no add runs ahead of the zeros
    __device__ __forceinline__ void clear(int np) const
    {
        __syncthreads();
#pragma unroll 1
        for (int t = threadIdx.x; t < np * C * HIST_ROW; t += 256) lds[t] = 0u;
        __syncthreads();
    }

    // sum np planes over the copies and write them to out[np][256]
    __device__ __forceinline__ void flush(int np, GLOBAL_AS unsigned *out) const
    {
        __syncthreads();
        const bool owned = gridDim.x == 1;
#pragma unroll 1
        for (int t = threadIdx.x; t < np * HIST_BINS; t += 256) {
            const unsigned *h = lds + (t >> 8) * C * HIST_ROW + (t & 255);
            unsigned s = 0;
#pragma unroll
            for (int k = 0; k < C; k++) s += h[k * HIST_ROW];
            if (owned) out[t] = s;
            else if (s) (void)__hip_atomic_fetch_add(out + t, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
};

__device__ __forceinline__ void hist_add(unsigned *h, unsigned bin, unsigned n)
{
    (void)__hip_atomic_fetch_add((lds_u32p)h + bin, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// Four neighbouring values of a lane: ONE add of 4 where they are equal, else an add each.  -DHIST_NO_MERGE: always an add each --
// the variant DESIGN 4.20 measures the merge against on a flat picture.
__device__ __forceinline__ void hist_add4(unsigned *h, unsigned b0, unsigned b1, unsigned b2, unsigned b3)
{
#ifndef HIST_NO_MERGE
    if (b0 == b1 && b1 == b2 && b2 == b3) {
        hist_add(h, b0, 4u);
        return;
    }
#endif
    hist_add(h, b0, 1u);
    hist_add(h, b1, 1u);
    hist_add(h, b2, 1u);
    hist_add(h, b3, 1u);
}

// ... of which the first nvalid < 4 are counted: an add each
__device__ __forceinline__ void hist_add_some(unsigned *h, unsigned b0, unsigned b1, unsigned b2, int nvalid)
{
    if (nvalid > 0) hist_add(h, b0, 1u);
    if (nvalid > 1) hist_add(h, b1, 1u);
    if (nvalid > 2) hist_add(h, b2, 1u);
}

// the four bytes of a dword: equal where the dword is itself rotated by a byte
__device__ __forceinline__ void hist_add_dword(unsigned *h, unsigned v)
{
#ifndef HIST_NO_MERGE
    if (v == __builtin_rotateleft32(v, 8)) {
        hist_add(h, v & 255u, 4u);
        return;
    }
#endif
    hist_add(h, v & 255u, 1u);
    hist_add(h, (v >> 8) & 255u, 1u);
    hist_add(h, (v >> 16) & 255u, 1u);
    hist_add(h, v >> 24, 1u);
}

// sixteen neighbouring bytes of a row, the first nvalid counted: one add of 16 where all are equal, else dword by dword
__device__ __forceinline__ void hist_add16(unsigned *h, const u32x4_t &v, int nvalid)
{
    if (nvalid == 16) {
#ifndef HIST_NO_MERGE
        if (v.x == __builtin_rotateleft32(v.x, 8) && v.x == v.y && v.y == v.z && v.z == v.w) {
            hist_add(h, v.x & 255u, 16u);
            return;
        }
#endif
#pragma unroll
        for (int i = 0; i < 4; i++) hist_add_dword(h, v[i]);
        return;
    }
    // (the piece at a row's end)
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int left = nvalid - 4 * i;
        if (left >= 4) hist_add_dword(h, v[i]);
        else hist_add_some(h, v[i] & 255u, (v[i] >> 8) & 255u, (v[i] >> 16) & 255u, left);
    }
}

// grid: x = pieces of 256 dwords of an output, y = the jobs of the launch.  dst: the launch's first output, `dwords` each
extern "C" __global__ void __launch_bounds__(256) vp8_hist_fill_kernel(uint8_t *dst, size_t dst_stride, int dwords)
{
    const int t = (int)(blockIdx.x * 256u + threadIdx.x);
    if (t < dwords) ((g_u32p)(dst + dst_stride * blockIdx.y))[t] = 0u;
}

// ---- pictures ----------------------------------------------------------------------------------------------------------------
#ifndef HIST_FRAME_LREP
#define HIST_FRAME_LREP 4            // (-DHIST_FRAME_LREP=1: the variant DESIGN 4.20 measures the lane copies against)
#endif
// |a - b| byte by byte
__device__ __forceinline__ unsigned hist_absdiff4(unsigned a, unsigned b)
{
    unsigned r = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int d = (int)((a >> (8 * i)) & 255u) - (int)((b >> (8 * i)) & 255u);
        r |= (unsigned)(d < 0 ? -d : d) << (8 * i);
    }
    return r;
}

template <int PL>
__device__ __forceinline__ u32x4_t hist_piece(const HistFrame &C, const HistFrame &R, bool pair, const HistFrameLaunch &L, int x, int y, int pw)
{
    u32x4_t v = hist_read16<PL>(C, L, x, y, pw);
    if (pair) {
        const u32x4_t r = hist_read16<PL>(R, L, x, y, pw);
#pragma unroll
        for (int i = 0; i < 4; i++) v[i] = hist_absdiff4(v[i], r[i]);
    }
    return v;
}

template <int PL>
__device__ __forceinline__ void hist_frame_plane(const HistLds<HIST_FRAME_LREP> &H, const HistFrame &C, const HistFrame &R, bool pair,
                                                 const HistFrameLaunch &L, GLOBAL_AS unsigned *out)
{
    const int pw = PL ? (L.dw + 1) >> 1 : L.dw, ph = PL ? (L.dh + 1) >> 1 : L.dh;
    int y0, y1;
    tensor_share(0, ph, L.S, (int)blockIdx.x, y0, y1);
    const int nrows = y1 - y0;
    H.clear(1);
    unsigned *h = H.plane(0);
    // two pieces a lane and round: both pieces' loads are in flight before the first add
#pragma unroll 1
    for (TensorWalk t((pw + 15) >> 4); t.row < nrows;) {
        const int n0 = min(16, pw - (t.col << 4));
        const u32x4_t a = hist_piece<PL>(C, R, pair, L, t.col << 4, y0 + t.row, pw);
        t.next();
        const bool two = t.row < nrows;
        int n1 = 0;
        u32x4_t b = {0u, 0u, 0u, 0u};
        if (two) {
            n1 = min(16, pw - (t.col << 4));
            b = hist_piece<PL>(C, R, pair, L, t.col << 4, y0 + t.row, pw);
            t.next();
        }
        hist_add16(h, a, n0);
        if (two) hist_add16(h, b, n1);
    }
    H.flush(1, out);
}

// grid: x = the workgroups that share a job's rows (L.S), y = the jobs of the launch.  raster / tiles: frame buffer 0 in its two
// forms (vp8_scale_kernel's); dst: the launch's first output
extern "C" __global__ void __launch_bounds__(256)
vp8_hist_frames_kernel(const uint8_t *__restrict__ raster, size_t fb_stride, const uint8_t *__restrict__ tiles, size_t tile_frame,
                       uint8_t *__restrict__ dst, size_t dst_stride, HistFrameLaunch L)
{
    __shared__ unsigned lds[HistLds<HIST_FRAME_LREP>::C * HIST_ROW];
    const HistLds<HIST_FRAME_LREP> H(lds);
    const HistFrameJob J = L.j[blockIdx.y];
    const bool pair = J.ref >= 0;
    const int rf = pair ? J.ref : J.fb;
    const HistFrame C = frame_of(raster, fb_stride, tiles, tile_frame, J.fb), R = frame_of(raster, fb_stride, tiles, tile_frame, rf);
    GLOBAL_AS unsigned *out = (GLOBAL_AS unsigned *)(dst + dst_stride * blockIdx.y);
    if (L.planes & VP8HIP_HIST_Y) { hist_frame_plane<0>(H, C, R, pair, L, out); out += HIST_BINS; }
    if (L.planes & VP8HIP_HIST_U) { hist_frame_plane<1>(H, C, R, pair, L, out); out += HIST_BINS; }
    if (L.planes & VP8HIP_HIST_V) hist_frame_plane<2>(H, C, R, pair, L, out);
}

// ---- slots -------------------------------------------------------------------------------------------------------------------
#define HIST_SLOT_LREP 1

// the MVMAG value of a cell's vector (col in the high half, row in the low one): the larger of the two components' magnitudes in
// whole pixels, rounded as the trace rounds a hop
__device__ __forceinline__ unsigned hist_mvmag(unsigned mv)
{
    const int px = (((int)mv >> 16) + 4) >> 3, py = ((int)(short)(mv & 0xffffu) + 4) >> 3;
    return (unsigned)min(max(px < 0 ? -px : px, py < 0 ? -py : py), 255);
}

// grid: x = the groups of macroblock rows of a frame, y = the jobs of the launch.  slot_base: IR slot 0, slot_bytes apart, records
// at o_mbx and vectors at o_mvs inside; dst: the launch's first output.  LDS: the sub-histograms of the planes asked for, then the
// staged records and vectors
extern "C" __global__ void __launch_bounds__(256)
vp8_hist_slots_kernel(const char *__restrict__ slot_base, size_t slot_bytes, size_t o_mbx, size_t o_mvs, uint8_t *__restrict__ dst, size_t dst_stride,
                      HistSlotLaunch L)
{
    extern __shared__ __attribute__((aligned(16))) unsigned hist_slot_lds[];
    const HistLds<HIST_SLOT_LREP> H(hist_slot_lds);
    const int f = (int)blockIdx.y, cols = L.mb_cols;
    const int np = __builtin_popcount(L.planes);
    const int m0 = (int)blockIdx.x * L.R, m1 = min(m0 + L.R, L.mb_rows);
    const unsigned qf = L.q[f];
    const bool read_mv = (L.planes & VP8HIP_HIST_MVMAG) && !((qf >> 28) & 1u);
    u32x4_t *lrec = (u32x4_t *)(hist_slot_lds + ((np * H.C * HIST_ROW + 3) & ~3));
    u32x4_t *lmvs = lrec + L.R * cols * 4;
    side_stage(slot_base + slot_bytes * (size_t)L.slot[f], o_mbx, o_mvs, cols, m0, m1, read_mv, lrec, lmvs);
    H.clear(np);

    const unsigned *rec = (const unsigned *)lrec, *mvs = (const unsigned *)lmvs;
    const int nq = (m1 - m0) * cols * 4;         // rows of four cells: four a macroblock
#pragma unroll 1
    for (int t = threadIdx.x; t < nq; t += 256) {
        SideCell c[4];
#pragma unroll
        for (int i = 0; i < 4; i++) side_cell(rec, mvs, t >> 2, (t & 3) * 4 + i, read_mv, L.planes, qf, c[i]);
        int p = 0;
#pragma unroll
        for (int b = 0; b <= HIST_SLOT_MVMAG; b++) {
            if (!((L.planes >> b) & 1u)) continue;       // (the same for every lane)
            unsigned v[4];
#pragma unroll
            for (int i = 0; i < 4; i++) v[i] = b == HIST_SLOT_MVMAG ? hist_mvmag(c[i].mv) : c[i].v[b] & 255u;
            hist_add4(H.plane(p++), v[0], v[1], v[2], v[3]);
        }
    }
    H.flush(np, (GLOBAL_AS unsigned *)(dst + dst_stride * f));
}

// ---- pool entries ------------------------------------------------------------------------------------------------------------
#define HIST_ENTRY_LREP 2

template <class Planes>
__device__ __forceinline__ void hist_entry_body(const uint8_t *__restrict__ pool, size_t pool_stride, uint8_t *__restrict__ dst, size_t dst_stride,
                                                const HistEntryLaunch &L)
{
    extern __shared__ __attribute__((aligned(16))) unsigned hist_entry_lds[];
    const HistLds<HIST_ENTRY_LREP> H(hist_entry_lds);
    const int np = __builtin_popcount(L.planes);
    int y0, y1;
    tensor_share(0, L.dh, L.S, (int)blockIdx.x, y0, y1);
    const unsigned p0 = (unsigned)y0 * (unsigned)L.dw, p1 = y1 > y0 ? (unsigned)y1 * (unsigned)L.dw : p0;      // (pixels of an entry: below 2^28)
    const GLOBAL_AS unsigned *src = (const GLOBAL_AS unsigned *)(pool + pool_stride * (size_t)L.idx[blockIdx.y]);
    H.clear(np);
#pragma unroll 1
    for (unsigned base = p0 + 4u * threadIdx.x; base < p1; base += 1024u) {
        const int nvalid = (int)min(4u, p1 - base);
        TraceQuad q;
        q.T = u32x4_t{0u, 0u, 0u, 0u};
        if (nvalid == 4) q.T = load4_dword_aligned(src + base);
        else {
#pragma unroll
            for (int i = 0; i < 3; i++)
                if (i < nvalid) q.T[i] = src[base + i];
        }
        int p = 0;
#pragma unroll
        for (int c = 0; c < Planes::N; c++) {
            if (!((L.planes >> c) & 1u)) continue;       // (the same for every lane)
            unsigned *h = H.plane(p++);
            const unsigned v[4] = {(unsigned)Planes::value(q, 0, c), (unsigned)Planes::value(q, 1, c), (unsigned)Planes::value(q, 2, c),
                                   (unsigned)Planes::value(q, 3, c)};
            if (nvalid == 4) hist_add4(h, v[0], v[1], v[2], v[3]);
            else hist_add_some(h, v[0], v[1], v[2], nvalid);
        }
    }
    H.flush(np, (GLOBAL_AS unsigned *)(dst + dst_stride * blockIdx.y));
}

// grid: x = the workgroups that share an entry's rows (L.S), y = the jobs of the launch.  pool: entry 0; dst: the launch's first
// output.  LDS: the sub-histograms of the planes asked for
#define HIST_ENTRY_KERNEL(NAME, PLANES)                                                                                                   \
    extern "C" __global__ void __launch_bounds__(256)                                                                                     \
    NAME(const uint8_t *__restrict__ pool, size_t pool_stride, uint8_t *__restrict__ dst, size_t dst_stride, HistEntryLaunch L)           \
    {                                                                                                                                     \
        hist_entry_body<PLANES>(pool, pool_stride, dst, dst_stride, L);                                                                   \
    }
HIST_ENTRY_KERNEL(vp8_hist_wear_kernel, WearPlanes)
HIST_ENTRY_KERNEL(vp8_hist_cover_kernel, CoverPlanes)
