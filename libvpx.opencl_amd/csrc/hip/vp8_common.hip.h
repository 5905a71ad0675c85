// Shared device-side definitions for the gfx950 VP8 pixel-path kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "vp8_ir.h"

// One frame of work as the kernels see it (device memory, one entry per job of a launch).
struct DevJob {
    vp8ir_frame_hdr hdr;          // 64 B
    const vp8ir_mbx *mbx;         // the slot's macroblock records (include/vp8_ir.h, the device form): 128 B each
    const int16_t  *blocks;       // ... and its block stream: 32 B per block with eob > 1
    const vp8ir_mv *mvs;
    uint8_t        *dst;
    const uint8_t  *ref[4];       // [1..3] = last / golden / alt-ref frame buffers (inter frames); [0] unused
    uint8_t        *tile;         // lane-per-row (key-frame) pipeline: the job's macroblock-tiled scratch frame (VP8_TILE_BYTES per macroblock)
    const uint8_t  *ref_tile[3];  // the TILED forms of ref[1..3] (null where a reference has none): vp8_inter_pred_tiles_kernel
    // 64 + 8*8 + 4*8 = 160 B
};
static_assert(sizeof(DevJob) == 160, "DevJob layout");

// Frame geometry common to all jobs of a launch (vp8ir_geom, flattened for kernel args).
struct DevGeom {
    int mb_cols, mb_rows;
    int aligned_w, aligned_h;
    int y_stride, uv_stride;
    int y_off, u_off, v_off;
};

// One plane of vp8hip_frames_scale_async (vp8_scale.hip), as the host's plan (vp8hip_scale.hip: vp8hip_scale_plan) left it
struct ScalePlane {
    int path, filt;               // SCALE_* below; filt: the path's filtered form
    int sw, sh, dw, dh;           // the plane's picture and its scaled size
    int aw, ah;                   // the aligned area every source coordinate is clamped to
    int dx, dy, x0, y0, maxx, maxy;   // 16.16 steps, first positions and clamps (POINT, BILIN8, BILIN16)
    int src_off, src_stride;      // raster form: the plane's origin in the frame buffer
    int tile_plane;               // tiled form: 0 luma, 1 U, 2 V
    int doff, dsize;              // the plane in a packed frame: offset and bytes
    int blk0;                     // first workgroup (blockIdx.x) of the plane
    int br;                       // output rows per workgroup (a band, its source rows staged in LDS); 0: read from the frame
    int nr, rw;                   // LDS slots per output row (source rows it reads), bytes per slot
    int adv_rows, adv_cols;       // 1024 destination bytes (a lane's step) as rows and columns of the plane: 1024 = adv_rows * dw + adv_cols
};
#define SCALE_COPY 0              // ScalePlane::path: ScalePlane's dispatch (scale.c:3702)
#define SCALE_DOWN2 1
#define SCALE_DOWN4 2
#define SCALE_DOWN8 3
#define SCALE_DOWN34 4
#define SCALE_DOWN38 5
#define SCALE_POINT 6             // ScalePlaneSimple
#define SCALE_BILIN8 7            // ScalePlaneBilinear's rows: 8-bit row fraction
#define SCALE_BILIN16 8           // ScalePlaneBilinearSimple
#define SCALE_FROM_RASTER 0       // ScaleLaunch::fb: the form a frame is read from
#define SCALE_FROM_TILES 1
#define SCALE_FROM_ZERO 2         // a frame buffer never written: its raster form would be zeros (and the pool need not exist)
#define SCALE_MAX_FRAMES 512      // frame buffers per launch (kernel arguments)
#define SCALE_MAX_LDS 65536       // LDS of a band
#define SCALE_WIN 4               // destination bytes per lane: an aligned dword
struct ScaleLaunch {
    ScalePlane p[3];
    int blocks, mb_cols;          // workgroups of a frame (gridDim.x); the frame's width in macroblocks
    int fb[SCALE_MAX_FRAMES];     // frame buffer << 2 | form (SCALE_FROM_*)
};

// One launch of vp8hip_frames_rgb_async (vp8_rgb.hip), as the host's plan (vp8hip_rgb.hip: rgb_plan) left it
#define RGB_PLANAR 0              // vp8hip_rgb::layout
#define RGB_PACKED3 1
#define RGB_PACKED4 2
#define RGB_U8 0                  // vp8hip_rgb::dtype
#define RGB_F16 1
#define RGB_F32 2
#define SCALE_FROM_PACKED 3       // RgbLaunch::fb's form: a packed I420 image of the scaled size (the call's scratch)
struct RgbLaunch {
    ScalePlane p[3];              // the SOURCE planes: aw, ah, rw, src_off, src_stride, tile_plane (of a packed image: aw = its width, src_off its offset)
    int w, h;                     // the output
    int br;                       // output rows per workgroup (even): br luma rows and br / 2 rows of each chroma plane in LDS
    int mb_cols;
    int vec;                      // every store of a lane is a whole aligned piece (w % 4 == 0 and dst, dst_stride aligned to the piece)
    int cy, k0;                   // channel at POSITION p of pixel = clamp255((cy * Y + k0 + cu[p] * (U - 128) + cv[p] * (V - 128)) >> 8)
    int cu[3], cv[3];             // (k0 = 128 - cy * yoff)
    float scale[3], bias[3];      // by position; float types
    int fb[SCALE_MAX_FRAMES];     // frame buffer << 2 | form (SCALE_FROM_*); SCALE_FROM_PACKED: frame k of the launch is image k of the scratch
};

// The element types of the tensors the side and residual kernels write (vp8_tensor_out.hip.h): vp8hip_side::mv_dtype, vp8hip_residual::dtype
#define TENSOR_I16 0
#define TENSOR_F16 1
#define TENSOR_F32 2
#define TENSOR_U8 3               // a byte, the value itself: vp8hip_trace_wear::dtype 0 (VP8HIP_WEAR_F16 / _F32 are TENSOR_F16 / _F32)

// One launch of vp8hip_frames_side_async (vp8_side.hip), as the host's plan (vp8hip_side.hip: side_plan) left it
#define SIDE_MAX_FRAMES 256       // slots per launch (kernel arguments)
#define SIDE_X_ANY 0              // SideLaunch::xmode: sx by the division; ...
#define SIDE_X_DISPLAY 1          // ... gw is the display width: the four outputs of a group share the cell x >> 2; ...
#define SIDE_X_NATIVE 2           // ... the native grid: the cell is x
struct SideLaunch {
    int gw, gh;                   // the output grid
    int dw, dh;                   // the size the grid is laid over: the display size, or the coded size for the native grid
    int mb_cols, mb_rows;
    int R;                        // macroblock rows a workgroup stages (a group); LDS = R * mb_cols * 128 bytes
    int S;                        // workgroups that share the output rows of a group (gridDim.x = groups * S)
    int xmode;                    // SIDE_X_*
    int mv_vec, info_vec;         // every store of a lane is a whole aligned piece (gw % 4 == 0 and destination, stride aligned to the piece)
    unsigned planes;              // VP8HIP_SIDE_* bits of the info tensor
    float scale[2];               // x, y; float types
    int slot[SIDE_MAX_FRAMES];    // IR slot of frame k of the launch
    unsigned q[SIDE_MAX_FRAMES];  // ... its header: the quantiser index of segment s in bits 7s .. 7s + 6, bit 28 = key frame
};

// One launch of vp8hip_frames_residual_async (vp8_residual.hip), as the host's plan (vp8hip_residual.hip: residual_plan) left it
#define RES_I420 0                // vp8hip_residual::layout
#define RES_PLANAR 1
#define RES_RUN 16                // macroblocks of a workgroup: a run of one macroblock row (records 2 KB + image 12.5 KB of LDS)
#define RES_MAX_FRAMES 128        // slots per launch (kernel arguments: 16 bytes each)
struct ResSlot {                  // what the kernel needs of a slot and its header as of the call
    int slot;
    unsigned q;                   // the quantiser index of segment s in bits 7s .. 7s + 6 (mb_init_dequantizer)
    unsigned d0, d1;              // y1dc, y2dc, y2ac, uvdc _delta_q as bytes of d0; uvac_delta_q in the low byte of d1
};
struct ResLaunch {
    int gw, gh;                   // the luma grid
    int dw, dh;                   // the size it is laid over: the display size, or the coded size for the native grid
    int cw, ch, dcw, dch;         // I420: the chroma grid and the size it is laid over
    int mb_cols, mb_rows;
    int runs;                     // runs of a macroblock row: (mb_cols + RES_RUN - 1) / RES_RUN
    int S;                        // workgroups that share the output rows of a run (gridDim.x = mb_rows * runs * S)
    int layout;                   // RES_*
    int y_vec, c_vec;             // every whole group of four of a luma / chroma plane is one aligned piece
    float scale[3];               // Y, U, V; float types
    ResSlot s[RES_MAX_FRAMES];
};

// One launch of vp8hip_frames_coef_async (vp8_coef.hip), as the host's plan (vp8hip_coef.hip) left it
#define COEF_DEQUANT 0            // vp8hip_coef::stage
#define COEF_LEVELS 1
#define COEF_CHANNELS 0           // vp8hip_coef::layout
#define COEF_INPLACE 1
#define COEF_RUN 32               // macroblocks of a workgroup: a run of one macroblock row (records 4 KB + image 27.3 KB of LDS)
#define COEF_PLANES 4             // Y, U, V, Y2: bit order of vp8hip_coef::planes
struct CoefLaunch {
    int mb_cols, mb_rows;
    int runs;                     // runs of a macroblock row: (mb_cols + COEF_RUN - 1) / COEF_RUN
    int stage, layout;            // COEF_*
    int zigzag;                   // CHANNELS: channel j is position zigzag[j], not j
    int nfreq;                    // CHANNELS: channels kept; INPLACE: 16
    unsigned planes;              // VP8HIP_COEF_* bits
    unsigned vec;                 // bit p: every whole group of four of plane p is one aligned piece
    float scale[COEF_PLANES];     // float types
    unsigned long long off[COEF_PLANES];      // where plane p begins in a frame's tensor, in elements
    ResSlot s[RES_MAX_FRAMES];
};

// One launch of vp8hip_frames_trace_async (vp8_trace.hip), as the host's plan (vp8hip_trace.hip) left it
#define TRACE_MAX_FRAMES 128      // jobs per launch (kernel arguments: 24 bytes each)
struct TraceJob {                 // a job and its slot's header as of the call
    int slot;
    int ref[3];                   // pool entries of last / golden / altref; -1: none
    int dst;                      // the pool entry written
    int key;                      // h.frame_type == 0: the identity, nothing read
};
struct TraceLaunch {
    int dw, dh;                   // the display size: the trace's grid
    int mb_cols, mb_rows;
    int R;                        // macroblock rows a workgroup stages (a group); LDS = R * mb_cols * 68 bytes
    int vec;                      // every store of a lane is a whole aligned piece (dw % 4 == 0 and pool, stride aligned to 16)
    TraceJob j[TRACE_MAX_FRAMES];
};

// What the readers of a trace pool share of a launch (vp8_trace_read.hip.h), as the host's plan (vp8hip_trace.hip: trace_grid) left it
struct TraceGrid {
    int gw, gh;                   // the output grid
    int S;                        // workgroups that share a frame's or job's output rows (gridDim.x)
    int dw, dh;                   // the display size it is laid over: the trace's grid, and what trace values are clamped to
    int vec;                      // every store of a lane is a whole aligned piece
    int xmode;                    // SIDE_X_DISPLAY (gw is the display width: sx = x) or SIDE_X_ANY
};

// One launch of a call that hands pool entries out as tensors (entry_tensor_body, vp8_trace_read.hip.h): vp8hip_trace_flow_async
// (vp8_trace.hip), vp8hip_trace_wear_async (vp8_trace_wear.hip) and vp8hip_trace_cover_async (vp8_trace_invert.hip)
#define FLOW_MAX_FRAMES 512       // pool entries per launch (kernel arguments)
struct EntryLaunch {
    TraceGrid g;
    unsigned planes;              // wear, cover: VP8HIP_WEAR_* / VP8HIP_COVER_* bits, plane c of the tensor where bit c is set, in bit order; flow: not read
    float scale[4];               // by plane (flow: x, y; wear: HOPS, INTRA, EDGE, CODED; cover: COUNT, SEEN); float types
    int idx[FLOW_MAX_FRAMES];     // pool entry of frame k of the launch
};

// One launch of vp8hip_trace_residual_async (vp8_trace_residual.hip), as the host's plan (vp8hip_trace.hip) left it
#define ANCHOR_MAX_FRAMES 128     // jobs per launch (kernel arguments: 12 bytes each)
struct AnchorJob {
    int fb;                       // the frame: frame buffer << 2 | form (SCALE_FROM_*), as of the call
    int trace;                    // the pool entry that holds its trace
    int anchor;                   // the anchor picture: frame buffer << 2 | form
};
struct AnchorLaunch {
    TraceGrid g;
    int mb_cols;
    int aw, ah;                   // the aligned area of the luma plane (chroma: half of it)
    int y_off, u_off, v_off, y_stride, uv_stride;    // the raster form: the planes' origins in a frame buffer and their strides
    int cy, k0;                   // RgbLaunch's: the byte at POSITION p = clamp255((cy * Y + k0 + cu[p] * (U - 128) + cv[p] * (V - 128)) >> 8)
    int cu[3], cv[3];
    float scale[3];               // by position; float types
    AnchorJob j[ANCHOR_MAX_FRAMES];
};

// One launch of vp8hip_trace_gather_async (vp8_trace_gather.hip), as the host's plan (vp8hip_trace.hip) left it
#define GATHER_MAX_JOBS 256       // jobs per launch (kernel arguments: 8 bytes each)
#define GATHER_PLANAR 0           // VP8HIP_GATHER_PLANAR, _CHANNELS_LAST
#define GATHER_CHANNELS_LAST 1
#define GATHER_NEAREST 0          // VP8HIP_GATHER_NEAREST, _BILINEAR
#define GATHER_BILINEAR 1
#define GATHER_RUN 256            // CHANNELS_LAST: outputs a workgroup takes, one lane each for the offsets
struct GatherJob {
    int trace;                    // the pool entry that holds the trace
    int src;                      // the source tensor
};
struct GatherLaunch {
    TraceGrid g;                  // CHANNELS_LAST: S = runs of GATHER_RUN outputs (gridDim.x), vec = every store AND load is a whole piece
    int sw, sh;                   // the source tensors' grid
    int C;                        // channels
    int cgroup;                   // PLANAR: channels a workgroup makes (gridDim.z groups of them)
    GatherJob j[GATHER_MAX_JOBS];
};

// One launch of vp8hip_trace_invert_async (vp8_trace_invert.hip): the fill and the scatter take the same one
#define INVERT_MAX_JOBS 256       // jobs per launch (kernel arguments: 8 bytes each)
struct InvertJob {
    int trace;                    // the pool entry read
    int dst;                      // the entry of the FIRST and of the COUNT pool written
};
struct InvertLaunch {
    int dw, dh;                   // the display size: the grid of the trace and of both outputs, and what trace values are clamped to
    int S;                        // workgroups that share a job's rows (gridDim.x)
    int vec;                      // the scatter's -DINVERT_LANE_QUADS variant: a lane's four trace dwords are one load (dw % 4 == 0 and pool, stride aligned to 16)
    int first_vec, count_vec;     // fill: the entries of that pool take whole 16-byte stores (pool, stride aligned to 16)
    InvertJob j[INVERT_MAX_JOBS];
};

// Where the planes of the context's frame buffers lie, for the kernels that read pictures and make no tensor of them
// (vp8_frame_read.hip.h): what a launch of the byte histograms, of the structural similarity, of the motion search and of its
// sub-pixel refinement begins with
struct FramePlanes {
    int dw, dh;                   // the display size
    int mb_cols, mb_rows;
    int y_off, u_off, v_off, y_stride, uv_stride;    // the raster form: the planes' origins in a frame buffer and their strides
};

// One launch of the byte histograms (vp8_hist.hip), as the host's plans (vp8hip_hist.hip) left it: vp8hip_frames_hist_async,
// vp8hip_slots_hist_async, vp8hip_trace_wear_hist_async and vp8hip_trace_cover_hist_async.  gridDim.x workgroups share a job; where
// that is more than one, vp8_hist_fill_kernel has run first and the workgroups add their counts with global atomics
#define HIST_MAX_JOBS 256         // jobs per launch (kernel arguments: 8 bytes each at most)
#define HIST_BINS 256
#define HIST_ROW 257              // dwords from one LDS sub-histogram to the next: copy k's bin b lies in bank (b + k) % banks
#define HIST_SLOT_MVMAG 6         // the plane of VP8HIP_HIST_MVMAG, behind the six of VP8HIP_SIDE_*
struct HistFrameJob {
    int fb;                       // the frame: frame buffer << 2 | form (SCALE_FROM_*), as of the call
    int ref;                      // the frame it is compared with, the same way; -1: none
};
struct HistFrameLaunch : FramePlanes {
    int S;                        // workgroups that share a job's rows (gridDim.x)
    unsigned planes;              // VP8HIP_HIST_Y | _U | _V
    HistFrameJob j[HIST_MAX_JOBS];
};
struct HistSlotLaunch {
    int mb_cols, mb_rows;
    int R;                        // macroblock rows a workgroup stages (a group: gridDim.x of them); LDS = histograms + R * mb_cols * 128 bytes
    unsigned planes;              // VP8HIP_SIDE_* bits and VP8HIP_HIST_MVMAG
    int slot[HIST_MAX_JOBS];      // IR slot of job k of the launch
    unsigned q[HIST_MAX_JOBS];    // ... its header, as SideLaunch::q holds it
};
struct HistEntryLaunch {
    int dw, dh;                   // the display size: an entry's grid
    int S;                        // workgroups that share an entry's rows (gridDim.x)
    unsigned planes;              // VP8HIP_WEAR_* / VP8HIP_COVER_* bits
    int idx[HIST_MAX_JOBS];       // pool entry of job k of the launch
};

// One launch of vp8hip_frames_ssim_async (vp8_ssim.hip), as the host's plan (vp8hip_ssim.hip) left it.  A plane's windows are cut
// into bands of SSIM_BAND_ROWS window rows and a band into pieces of SSIM_BAND_COLS window columns; a job's pieces, the planes asked
// for one after the other, are dealt to the gridDim.x workgroups that share the job.  Where that is more than one and scores are
// asked for, vp8_ssim_fill_kernel has run first and the workgroups add their sums with global atomics
#define SSIM_MAX_JOBS 256         // jobs per launch (kernel arguments: 8 bytes each)
#define SSIM_BAND_ROWS 16         // window rows a piece owns: it stages SSIM_BAND_ROWS + 1 cell rows, the last one the halo
#define SSIM_BAND_COLS 63         // window columns a piece owns: it stages SSIM_BAND_COLS + 1 cell columns, the last one the halo
#define SSIM_F16 1                // VP8HIP_SSIM_F16, _F32
#define SSIM_F32 2
struct SsimPlane {                // a plane asked for, in bit order
    int pl;                       // 0 Y, 1 U, 2 V
    int nwx, nwy;                 // its windows
    int px;                       // pieces a band is cut into
    int first;                    // the job's pieces before this plane's
    int map_off;                  // elements of a job's map before this plane's
};
struct SsimLaunch : FramePlanes {
    int S;                        // workgroups that share a job's pieces (gridDim.x)
    int np;                       // planes asked for
    int pieces;                   // of a job, all planes
    int scores;                   // 1: scores are written
    int map_dtype;                // 0: no map; SSIM_F16 / SSIM_F32
    SsimPlane p[3];
    HistFrameJob j[SSIM_MAX_JOBS];    // (ref is never -1)
};
struct SsimFill {                 // what vp8_ssim_fill_kernel writes into every job's scores: {0, count} per plane
    int np;
    long long count[3];
};

// One launch of vp8hip_frames_motion_async (vp8_motion.hip), as the host's plan (vp8hip_motion.hip) left it.  A workgroup owns one
// macroblock of one job: it stages the search window -- `rows` rows of `pitch` dwords of the edge-replicated reference picture,
// its first byte the candidate (cy - d, cx - d) -- and the block, and deals the candidates to its lanes as items of MOTION_ROWS
// candidate rows by four candidate columns: `groups` x `nq` of them
#define MOTION_MAX_JOBS 256       // jobs per launch (kernel arguments: 8 bytes each)
#define MOTION_MAX_D 64
#define MOTION_ROWS 4             // candidate rows an item takes: a window row in registers serves up to four of them
#define MOTION_SAD 1              // VP8HIP_MOTION_*
#define MOTION_SAD0 2
#define MOTION_SSE 4
#define MOTION_VAR 8
#define MOTION_SRCVAR 16
struct MotionLaunch : FramePlanes {  // (dw, dh are not read: the search is over the coded area)
    int d;                        // the distance, 1..MOTION_MAX_D
    int nq, groups;               // items across (four candidate columns each) and down (MOTION_ROWS candidate rows each)
    int pitch, rows;              // the window in LDS: dwords per row (nq + 4 at least) and rows (MOTION_ROWS * groups + 15)
    int spb;                      // sad_per_bit; 0: no cost term
    unsigned planes;              // MOTION_* bits of the stats; 0: none
    int mv, centre;               // 1: vectors are written / centres are read
    unsigned short cost[2][2 * MOTION_MAX_D + 2];    // [0]: by row, [1]: by column, index = candidate - centre + d
    HistFrameJob j[MOTION_MAX_JOBS];    // (ref is never -1)
};

// One launch of vp8hip_frames_subpel_async (vp8_subpel.hip), as the host's plan (vp8hip_subpel.hip) left it.  A wave owns one
// macroblock of one job, SUBPEL_WAVES of them share a workgroup.  The cost table is not here: it lies in the context's device copy,
// sent there in pieces that come with launches of vp8_subpel_table_kernel
#define SUBPEL_MAX_JOBS 256       // jobs per launch (kernel arguments: 8 bytes each)
#define SUBPEL_WAVES 4            // macroblocks (waves) a workgroup
#define SUBPEL_MAX_RANGE 1023     // the largest cost_range: the reference's mv_max
#define SUBPEL_TABLE_ENTRIES (2 * (2 * SUBPEL_MAX_RANGE + 1))     // of the context's copy: 8188 bytes
#define SUBPEL_TABLE_PIECE 1792   // entries a launch of vp8_subpel_table_kernel carries
#define SUBPEL_VAL 1              // VP8HIP_SUBPEL_*
#define SUBPEL_VAR 2
#define SUBPEL_SSE 4
#define SUBPEL_VAR0 8
struct SubpelLaunch : FramePlanes {  // (dw, dh are not read: the blocks are those of the coded area)
    int precision;                // 2: the half-pixel stage alone; 4: both stages
    int epb;                      // error_per_bit; 0: no cost term (the table and the reference vectors are not read)
    int R;                        // cost_range: a row of the table has 2 R + 1 entries
    unsigned planes;              // SUBPEL_* bits of the stats; 0: none
    int mv, start, ref;           // 1: vectors are written / starts are read / reference vectors are read
    HistFrameJob j[SUBPEL_MAX_JOBS];    // (ref is never -1)
};
struct SubpelTablePiece {
    int first, n;                 // entries first .. first + n - 1 of the copy
    unsigned short v[SUBPEL_TABLE_PIECE];
};
// One launch of vp8hip_frames_tfilter_async (vp8_tfilter.hip), as the host's plan (vp8hip_tfilter.hip) left it.  A workgroup owns one
// macroblock of one job and loops over the job's sources; a job's sources lie in ref[roff .. roff + count - 1], copied there pair
// by pair (jobs that share pairs each have their own copy), so a launch takes jobs until either array is full
#define TFILTER_MAX_JOBS 96       // jobs per launch (kernel arguments: 16 bytes each)
#define TFILTER_MAX_REFS 480      // sources per launch (4 bytes each): 32 jobs of 15 at least
#define TFILTER_MAX_COUNT 15      // sources a job: the reference's arnr_max_frames
#define TFILTER_THREADS 128       // lanes 0..63: the luma block, four pixels each; 64..95: U and V; all of them stage and filter rows
struct TfilterJob {
    int fb;                       // the centre: frame buffer << 2 | form, as of the call
    int first;                    // its first pair in the caller's list: where its vectors and errors lie
    int count;                    // 1..TFILTER_MAX_COUNT
    int roff;                     // its first source in TfilterLaunch::ref
};
struct TfilterLaunch : FramePlanes {
    int strength;                 // 0..6
    int filter;                   // 0: six-tap, 1: bilinear
    unsigned lo, hi;              // the thresholds of the weight: err < lo: 2, err < hi: 1, else 0
    int mv, err, dst, cnt;        // 1: vectors are read / errors are read / pictures are written / counts are written
    TfilterJob j[TFILTER_MAX_JOBS];
    int ref[TFILTER_MAX_REFS];    // the sources: frame buffer << 2 | form
};
// One launch of vp8hip_frames_quant_async (vp8_quant.hip), as the host's plan (vp8hip_quant.hip) left it.  A workgroup owns one
// macroblock of one job.  A job names one of the launch's tables: what vp8hip_quant_factors gave for the job's qindex, as it stands,
// then the three zero-bin extras; jobs of one qindex share a table, so a launch takes jobs until either array is full
#define QUANT_MAX_JOBS 160        // jobs per launch (kernel arguments: 12 bytes each)
#define QUANT_MAX_TABLES 8        // distinct qindex values per launch (176 bytes each)
#define QUANT_THREADS TFILTER_THREADS    // the prediction is vp8_mc_pred.hip.h's: the same lanes own the same pixels
#define QUANT_TABLE_SHORTS 88     // 84 of vp8hip_quant_table, 3 extras (Y1, Y2, UV), 1 unused
#define QUANT_ERRY 1              // VP8HIP_QUANT_*
#define QUANT_ERRY2 2
#define QUANT_ERRUV 4
#define QUANT_EOBS 8
#define QUANT_RECSSE 16
struct QuantJob {
    int fb, ref;                  // the source and the reference picture: frame buffer << 2 | form, as of the call
    int table;                    // its table in QuantLaunch::t
};
struct QuantLaunch : FramePlanes {
    int filter;                   // 0: six-tap, 1: bilinear
    int fast;                     // 0: the regular quantiser, 1: the fast one
    int levels;                   // coef holds 1: qcoeff, 0: dqcoeff
    unsigned planes;              // QUANT_* bits of the stats; 0: none
    int mv, coef, eob, rec;       // 1: vectors are read / coefficients, eobs, reconstructions are written
    short t[QUANT_MAX_TABLES][QUANT_TABLE_SHORTS];
    QuantJob j[QUANT_MAX_JOBS];
};
// One launch of vp8hip_frames_intra_async (vp8_intra_enc.hip), as the host's plan (vp8hip_intra.hip) left it.  A WORKGROUP owns one
// job and walks its macroblocks as a wavefront: step s holds the macroblocks (r, c) with c + 2 r == s, dealt to the workgroup's waves,
// a workgroup barrier between steps.  Rows are walked in bands of INTRA_BAND; the tables are vp8hip_quant_staged_table's, one per
// distinct qindex; the mode costs ride in the arguments, so a launch takes jobs until either array is full
#define INTRA_MAX_JOBS 256        // jobs per launch (kernel arguments: 4 bytes each)
#define INTRA_MAX_TABLES 4        // distinct qindex values per launch (176 bytes each)
#define INTRA_WAVES 8             // waves a workgroup: macroblocks of a step coded at the same time
#define INTRA_THREADS (64 * INTRA_WAVES)
#define INTRA_BAND 68             // macroblock rows a band: 1080p is one band; LDS holds a ring of four bottom lines per row of a band
#define INTRA_LINE_WORDS 9        // a macroblock's bottom line (or right column): Y 16, U 8, V 8 bytes, then its four sub-block modes
#define INTRA_RD16 1              // VP8HIP_INTRA_*
#define INTRA_RD4 2
#define INTRA_RATE 4
#define INTRA_EOBS 8
#define INTRA_RECSSE 16
struct IntraLaunch : FramePlanes {
    int fast;                     // 0: the regular quantiser, 1: the fast one
    int levels;                   // coef holds 1: qcoeff, 0: dqcoeff
    unsigned planes;              // INTRA_* bits of the stats; 0: none
    int coef, eob, rec, modes;    // 1: coefficients, eobs, reconstructions, modes are written
    int rdmult, rddiv;            // RDCOST's two
    int bmode_last;               // the last sub-block mode tried, 0..9
    int no_bpred;                 // 1: step 3 is left out
    unsigned short mbmode_cost[6];       // DC, V, H, TM, B_PRED; one unused
    unsigned short bmode_cost[1000];     // [above][left][mode]
    short t[INTRA_MAX_TABLES][QUANT_TABLE_SHORTS];
    int j[INTRA_MAX_JOBS];        // the source: frame buffer << 2 | form, as of the call, and in bits 28..29 its table
};
// the five launches' layout in the kernels' arguments: the base takes 36 bytes and the first member lies right behind it (offsetof
// past a base of plain ints is what the warning calls conditionally supported: it is supported here)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winvalid-offsetof"
static_assert(sizeof(FramePlanes) == 36 && sizeof(HistFrameLaunch) == 2092 && sizeof(SsimLaunch) == 2176 && sizeof(MotionLaunch) == 2640, "");
static_assert(sizeof(SubpelLaunch) == 2112 && sizeof(SubpelTablePiece) == 3592, "");
static_assert(offsetof(HistFrameLaunch, S) == 36 && offsetof(SsimLaunch, S) == 36 && offsetof(MotionLaunch, d) == 36, "");
static_assert(offsetof(SubpelLaunch, precision) == 36, "");
static_assert(sizeof(TfilterLaunch) == 3524 && offsetof(TfilterLaunch, strength) == 36, "");
static_assert(sizeof(QuantLaunch) == 3396 && offsetof(QuantLaunch, filter) == 36 && offsetof(QuantLaunch, t) == 68, "");
#pragma clang diagnostic pop

#define WAVE 64

// Macroblock tiles of the one-MB-row-per-lane pipeline (vp8_keyframe_simt.hip has the layout): three 128-byte lines per macroblock.
#define VP8_TILE_BYTES 384

// Pointers that come out of a DevJob (i.e. out of memory) are generic to the compiler, which then
// emits FLAT loads/stores: those count on lgkmcnt as well as vmcnt, so every LDS wait would also
// wait for the global prefetches and the frame write-out.  Casting to the global address space
// makes them global_load/global_store (vmcnt only).
#define GLOBAL_AS __attribute__((address_space(1)))
typedef GLOBAL_AS unsigned char *g_u8p;
typedef GLOBAL_AS const unsigned char *g_cu8p;
typedef GLOBAL_AS unsigned int *g_u32p;
typedef GLOBAL_AS const unsigned int *g_cu32p;
typedef GLOBAL_AS const short *g_cs16p;

// ---- intra-workgroup progress flags in LDS ------------------------------------------------
// A wave publishes "(row sequence number << 16) | MBs finished in that row"; finishing a row
// publishes (seq+1) << 16.  All waves of a workgroup live on one CU.
//
// Two flavours, chosen by where the handed-over DATA lives:
//  * data in LDS (recon kernel's line buffers): a wave's LDS operations are executed in issue
//    order, so "write data; write flag" / "read flag; read data" need NO s_waitcnt at all -- only
//    the compiler must be kept from reordering.  In particular the publisher does not wait for its
//    outstanding global stores (frame write-out) and the consumer does not drain its prefetches.
//  * data in global memory (loop-filter kernel's context rows): the publisher must have its stores
//    acknowledged (s_waitcnt vmcnt(0)) before the flag store; same CU => same L1/L2, so workgroup
//    scope needs no cache maintenance (LLVM AMDGPU memory model, non-tgsplit mode).
__device__ __forceinline__ void compiler_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

#ifndef VP8_POLL_SLEEP
#define VP8_POLL_SLEEP 1   // s_sleep units (64 clocks) between polls of a progress flag
#endif
__device__ __forceinline__ void wg_wait_ge(int *flag, int value)
{
    while (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < value)
        __builtin_amdgcn_s_sleep(VP8_POLL_SLEEP);
    compiler_fence();
}

__device__ __forceinline__ void wg_publish_lds(int *flag, int value, int lane)
{
    compiler_fence();
    if (lane == 0)
        __hip_atomic_store(flag, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__device__ __forceinline__ void wg_publish_global(int *flag, int value, int lane)
{
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    compiler_fence();
    if (lane == 0)
        __hip_atomic_store(flag, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// Lanes of one wave exchanging data through LDS: the hardware issues a wave's LDS operations in
// order, but the COMPILER only promises per-thread ordering and may move one lane's load above
// another lane's store.  This is the (instruction-free) fence that pins the order.
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

__device__ __forceinline__ int wave_sum(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
    return v;
}

// quantiser lookups (vp8/common/quant_common.c:14-37); VP8 format constants
// (the values as macros: vp8hip_dequant_factors, vp8hip_coef.hip, keeps the same two tables on the host)
#define VP8_DC_Q_VALUES \
    4, 5, 6, 7, 8, 9, 10, 10, 11, 12, 13, 14, 15, 16, 17, 17, 18, 19, 20, 20, 21, 21, 22, 22, 23, 23, 24, 25, 25, 26,  \
    27, 28, 29, 30, 31, 32, 33, 34, 35, 36, 37, 37, 38, 39, 40, 41, 42, 43, 44, 45, 46, 46, 47, 48, 49, 50, 51, 52,    \
    53, 54, 55, 56, 57, 58, 59, 60, 61, 62, 63, 64, 65, 66, 67, 68, 69, 70, 71, 72, 73, 74, 75, 76, 76, 77, 78, 79,    \
    80, 81, 82, 83, 84, 85, 86, 87, 88, 89, 91, 93, 95, 96, 98, 100, 101, 102, 104, 106, 108, 110, 112, 114, 116,      \
    118, 122, 124, 126, 128, 130, 132, 134, 136, 138, 140, 143, 145, 148, 151, 154, 157
#define VP8_AC_Q_VALUES \
    4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33,  \
    34, 35, 36, 37, 38, 39, 40, 41, 42, 43, 44, 45, 46, 47, 48, 49, 50, 51, 52, 53, 54, 55, 56, 57, 58, 60, 62, 64,    \
    66, 68, 70, 72, 74, 76, 78, 80, 82, 84, 86, 88, 90, 92, 94, 96, 98, 100, 102, 104, 106, 108, 110, 112, 114, 116,   \
    119, 122, 125, 128, 131, 134, 137, 140, 143, 146, 149, 152, 155, 158, 161, 164, 167, 170, 173, 177, 181, 185,      \
    189, 193, 197, 201, 205, 209, 213, 217, 221, 225, 229, 234, 239, 245, 249, 254, 259, 264, 269, 274, 279, 284
__constant__ static const unsigned short k_dc_q[128] = { VP8_DC_Q_VALUES };
__constant__ static const unsigned short k_ac_q[128] = { VP8_AC_Q_VALUES };

// ---- in-kernel stamps (diagnostic builds only: -DVP8_STAMPS; never in the product build) ------------------
// Where a lane-per-row kernel's step spends its cycles: STAMP(i) adds the shader cycles since the previous stamp
// to bucket i (wave-uniform, kept in SGPRs); the first wave of the grid adds its buckets to a device array of its
// own that no kernel reads (MI355X guide, "In-kernel stamps").  Shares only -- the build itself runs slower.
// ---- granule hand-over between the workgroups of a frame (vp8_recon_xcu_kernel / vp8_loopfilter_xcu_kernel) ----
// A granule is 4 bytes of data and the tag (launch counter) of the launch that wrote it in one 8-byte word, stored and
// loaded with one relaxed agent-scope access: the tag is the progress flag, there is no separate flag and no fence.
// A bounded poll turns a broken hand-over into an error status instead of a hang: the first poll that runs out sets
// *err (host-visible) and marks the launch in vp8_gran_broken; from then on every wait of that launch gives up after one
// look, so the kernel drains in milliseconds instead of repeating the full budget per macroblock.
typedef unsigned long long u64;
typedef GLOBAL_AS u64 *g_u64p;
extern __device__ unsigned int vp8_gran_broken;     // tag of the last launch in which a hand-over timed out (vp8hip.hip)
__device__ __forceinline__ void gran_store(g_u64p p, unsigned int data, unsigned int tag)
{
    __hip_atomic_store(p, (u64)data | ((u64)tag << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ u64 gran_load(g_u64p p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// v: what an earlier gran_load of *p returned; polls only if that was too early
__device__ __forceinline__ unsigned int gran_wait(g_u64p p, u64 v, unsigned int tag, int *err, int code)
{
    int budget = 0;
    for (int n = 0; (unsigned int)(v >> 32) != tag; ++n) {
        if (n == 0) budget = __hip_atomic_load(&vp8_gran_broken, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == tag ? 1 : (1 << 22);
        if (n >= budget) {
            *err = code;
            __hip_atomic_store(&vp8_gran_broken, tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            break;
        }
        __builtin_amdgcn_s_sleep(VP8_POLL_SLEEP);
        v = gran_load(p);
    }
    return (unsigned int)v;
}

#ifdef VP8_STAMPS
#define VP8_NSTAMPS 16
extern __device__ unsigned long long vp8_stamps_recon[VP8_NSTAMPS], vp8_stamps_lf[VP8_NSTAMPS];
#define STAMP_DECL unsigned long long st_acc[VP8_NSTAMPS]; unsigned long long st_last; \
    for (int i_ = 0; i_ < VP8_NSTAMPS; i_++) st_acc[i_] = 0; \
    { __builtin_amdgcn_sched_barrier(0); asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(st_last) :: "memory"); __builtin_amdgcn_sched_barrier(0); }
#define STAMP(i) { unsigned long long t_; __builtin_amdgcn_sched_barrier(0); \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_) :: "memory"); __builtin_amdgcn_sched_barrier(0); \
    st_acc[i] += t_ - st_last; st_last = t_; }
#define STAMP_FLUSH(arr) if (blockIdx.x == 0 && threadIdx.x == 0) { for (int i_ = 0; i_ < VP8_NSTAMPS; i_++) atomicAdd(&arr[i_], st_acc[i_]); }
#else
#define STAMP_DECL
#define STAMP(i)
#define STAMP_FLUSH(arr)
#endif
