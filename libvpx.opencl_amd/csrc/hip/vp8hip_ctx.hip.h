// Internal to libvp8hip.so: the context behind include/vp8hip.h's opaque handle, shared by the shim's translation units --
//   vp8hip.hip          context, pools, IR slots (upload / copy / fetch), frame buffers, statistics
//   vp8hip_launch.hip   vp8hip_decode: which kernels a launch runs; the two forms a frame buffer has on the device
//   vp8hip_entropy.hip  vp8hip_entropy_decode
//   vp8hip_postproc.hip vp8hip_postproc, vp8hip_mfqe
//   vp8hip_visualize.hip vp8hip_visualize
//   vp8hip_scale.hip, vp8hip_rgb.hip, vp8hip_side.hip, vp8hip_residual.hip, vp8hip_coef.hip   vp8hip_frames_scale_async, _rgb_async,
//                       _side_async, _residual_async, _coef_async: frames, and what the slots hold beside them, as tensors in the
//                       caller's device memory
//   vp8hip_trace.hip    vp8hip_frames_trace_async: accumulated motion in a pool in the caller's device memory (vp8_trace.hip), and
//                       the pool's readers vp8hip_trace_flow_async (vp8_trace.hip), vp8hip_trace_residual_async
//                       (vp8_trace_residual.hip) and vp8hip_trace_gather_async (vp8_trace_gather.hip); vp8hip_frames_wear_async and
//                       vp8hip_trace_wear_async: what happened along the trace, in a pool of its own, and its entries as tensors
//                       (vp8_trace_wear.hip)
//   vp8hip_hist.hip     vp8hip_frames_hist_async, vp8hip_slots_hist_async, vp8hip_trace_wear_hist_async, vp8hip_trace_cover_hist_async:
//                       byte histograms of pictures, slots and pool entries (vp8_hist.hip)
//   vp8hip_ssim.hip     vp8hip_frames_ssim_async: the structural similarity of picture pairs (vp8_ssim.hip)
//   vp8hip_motion.hip   vp8hip_frames_motion_async: full-search block motion between picture pairs (vp8_motion.hip)
//   vp8hip_subpel.hip   vp8hip_frames_subpel_async: the sub-pixel refinement of such vectors (vp8_subpel.hip)
//   vp8hip_handover.hip what those calls share: the checks of their lists, of picture pairs and of destinations, and the planes'
//                       geometry for the four calls that read picture pairs (hist, ssim, motion, subpel)
// and vp8hip_res.hip.h: the owning types of the context's buffers, events and streams.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "vp8hip.h"
#include "vp8_common.hip.h"
#include "vp8hip_res.hip.h"

#define VP8HIP_STATS_RING 32
#define VP8HIP_NBUF 4          // device job tables in rotation (a launch's table may still be read while the next one is staged)
#ifdef VP8_STAMPS
#define VP8HIP_SCHED_WORDS (16 + 16384 + 4 * 4096)     // + the diagnostic builds' log: four words per wave
#else
#define VP8HIP_SCHED_WORDS (16 + 16384)     // vp8_keyframe_kernel: two work counters, one arrival counter per SIMD of the device
#endif

// An IR slot: one frame's macroblock data in the DEVICE FORM of include/vp8_ir.h -- [pad 128][mbx: nmb x 128][blocks: up to
// nmb x 24 x 32][mvs: nmb x 64] in one device block (vp8hip_ctx::slot_block_dev + slot * slot_bytes) -- and, once mapped, pinned
// host staging of the same layout that a feeder fills and one copy sends.  The dense view (vp8hip_ir_map: what the oracle and
// the tests speak) is host memory only; vp8hip_ir_upload converts it on the host.
struct Slot {
    vp8ir_mbx *d_mbx = nullptr; int16_t *d_blocks = nullptr; vp8ir_mv *d_mvs = nullptr;
    PinnedBuf<char> h_block;                           // pinned staging, allocated on first map: same offsets as the device block
    vp8ir_frame_hdr *h_hdr = nullptr; vp8ir_mbx *h_mbx = nullptr; int16_t *h_blocks = nullptr; vp8ir_mv *h_mvs = nullptr;
    HeapBuf<char> h_dense; vp8ir_mb *h_mbs = nullptr; int16_t *h_coef = nullptr;   // the dense view (pageable), allocated on first vp8hip_ir_map
    vp8ir_frame_hdr hdr_copy = {};                     // header as of the last upload / copy / entropy launch (host side, for job setup)
    size_t nblocks = 0;                                // blocks in the device stream, as far as the host knows (NBLOCKS_UNKNOWN: written on the device)
};
#define NBLOCKS_UNKNOWN ((size_t)-1)

// Tuning / test knobs, read from the environment by vp8hip_configure (never per launch):
//   VP8HIP_RECON=simt|wave     force one of the two kernel families whatever the launch's size
//   VP8HIP_SIMT_LGG=1..6       lane-per-row kernels: lanes per strand (log2); VP8HIP_SIMT_WAVES=n  at most n waves per launch
//   VP8HIP_WG_PER_CU, VP8HIP_XCU, VP8HIP_XCU_S, VP8HIP_XCU_NW, VP8HIP_RECON_NW, VP8HIP_LF_NW   wave-per-row family shapes
//   VP8HIP_EAGER_RASTER=1      large launches produce the raster form of their frames at once (default: when something asks for it)
//   VP8HIP_D2H_STREAMS=1..4    a batch download goes in that many pieces on streams of their own (default 2)
//   VP8HIP_DIRECT_DOWNLOAD=0   batch downloads of tiled frames go through the raster form in HBM and a copy (default: the tiled ->
//                              raster pass writes the page-locked destination itself); VP8HIP_DOWNLOAD_BLOCKS=n  its workgroups
//   VP8HIP_INTER_SPLIT=N       launches of up to N frames with inter frames among them run vp8_inter_mb_kernel first (default 384; 0:
//                              never).  It shortens a frame's critical path (1080p P frames, 1..16 per launch: recon 0.91 -> 0.46-0.56
//                              ms; 128: 1.56 -> 1.45) and costs throughput in launches that fill the chip anyway (512: 3.82 -> 4.03)
#define VP8HIP_TILE_FRONT 4096
struct Knobs {
    int recon_force = 0;   // 0 automatic, 1 lane-per-row, 2 wave-per-row
    int md5_pack_from = 0; // VP8HIP_MD5_PACK_FROM: batches of this many tiled frames and more are hashed from a packed copy (vp8hip.hip: fetch_impl)
    int pred_tiles = 0;    // VP8HIP_PRED_TILES: 1 (default) a large launch whose references are all there as tiles, and not all as raster frames,
                           // predicts from the tiles; 2: whenever all are there as tiles; 0: never (the raster form is made first)
    int inter_split = 0, eager_raster = 0, direct_download = 0, download_blocks = 0, d2h_prio = 0, d2h_streams = 0;
    int lgG = 0, simt_waves = 0, wg_per_cu = 0, xcu = 0, xcu_S = 0, xcu_NW = 0, recon_nw = 0, lf_nw = 0;
};

// WHO OWNS WHAT.  Every buffer, event and stream of a context is a member of an owning type (vp8hip_res.hip.h): deleting the
// context -- vp8hip_destroy, a failure in vp8hip_create -- gives all of it back, and nothing is freed by hand anywhere.  Members
// are destroyed last to first, so the streams come first here: buffers and events go while the streams still exist, the main
// stream goes last.  A buffer that grows does so through Buf::grow, behind the wait its call site makes.
// WHAT SURVIVES A RECONFIGURATION.  vp8hip_configure gives back what is shaped by the geometry or the counts (free_pools in
// vp8hip.hip): the raster, tile and block pools, the slots with their stagings, the granule buffers and the intra flags.
// Everything else stays and is reused: job and conversion tables, digest buffers, the packed staging and the RGB scratch (caches:
// vp8hip_drop_staging), the entropy decoder's input sets, the MFQE and visualizer stagings, all streams and events -- and the
// post-processing tables with pp_rv_loaded: the caller's noise state outlives a reconfiguration too (vp8/common/postproc.c keeps
// postproc_state.noise across vp8_alloc_frame_buffers) and only sends the noise table again when q changes.
struct vp8hip_ctx {
    int device = 0;
    Knobs knobs;
    Stream stream;
    // batch download of whole frame buffers on a stream of its own (vp8hip_frames_download_async): PCIe is full duplex, the next
    // batch's uploads run beside it; in up to four pieces on streams of their own (a copy engine each)
    Stream stream_d2h, stream_d2h_more[3];
    Stream stream_h2d;             // vp8hip_entropy_decode: a launch's input
    // timing events of the last VP8HIP_STATS_RING launches: [0..3] on the main stream around recon / loop filter /
    // extend, [4..5] around the tiled -> raster pass on whichever stream it ran
    Event evr[VP8HIP_STATS_RING][6];
    bool evr_tiled[VP8HIP_STATS_RING] = {}; vp8hip_stats evr_stats[VP8HIP_STATS_RING] = {};
    long ncalls = 0;
    Event ev_jobs2[VP8HIP_NBUF];   // the job table staged in h_jobs2[k] has been copied
    int parity = 0;                // job table used by the next launch
    char err[256] = "";
    // geometry
    int width = 0, height = 0;
    vp8ir_geom geom = {};
    DevGeom dg = {};
    int nmb = 0;
    // pools.  A frame buffer has TWO forms on the device (vp8hip_launch.hip): the raster form -- the reference's YV12 layout with
    // its borders, fb[i] -- and the tiled form the lane-per-row kernels write -- macroblock-window tiles, fb_tiles[i], allocated
    // with the first large launch --, and fb_state[i] says which of them hold the frame.  Whoever needs a form the frame is not
    // in asks for it (vp8hip_need_raster): the conversion runs when something reads the frame as raster, not after every launch.
    std::vector<uint8_t *> fb, fb_tiles;
    std::vector<uint8_t> fb_state;
    std::vector<Slot> slots;
    DevBuf<uint8_t> fb_block; DevBuf<char> slot_block_dev;
    uint8_t *tile_block = nullptr; size_t tile_frame = 0;   // the tiled forms of all frame buffers (tile_frame bytes each) + the dummy tile
    DevBuf<uint8_t> tile_alloc;                      // ... as allocated: VP8HIP_TILE_FRONT bytes in front of tile_block (the tile-reading predictor's loads left of a tile row)
    DevBuf<DevJob> d_conv_jobs; PinnedBuf<DevJob> h_conv_jobs; Event ev_conv;    // job table of a tiled -> raster pass
    size_t slot_bytes = 0, o_mbx = 0, o_blocks = 0, o_mvs = 0, cap_blocks = 0;   // slot layout; cap_blocks = nmb * 24 (pooled: 0)
    // vp8hip_configure_pooled: the slots have no block streams of their own; the device's entropy decoder takes the blocks' room out
    // of this pool, chunk_blocks blocks at a time (pool_chunks chunks + one that takes what no longer fits); *d_pool_ctr = chunks taken
    DevBuf<char> pool; DevBuf<unsigned int> d_pool_ctr; unsigned int pool_chunks = 0, chunk_blocks = 0;
    // job staging
    // (device tables and page-locked stagings in rotation: a caller may queue VP8HIP_NBUF launches before it has to wait for the
    // device to have taken the first one's table -- behind an entropy launch of a quarter of a second, say)
    DevBuf<DevJob> d_jobs2[VP8HIP_NBUF]; PinnedBuf<DevJob> h_jobs2[VP8HIP_NBUF]; DevJob *d_jobs = nullptr, *h_jobs = nullptr;   // d_jobs / h_jobs = those of the call
    // launch configuration
    int num_cu = 0, max_lds = 0;
    int recon_nw = 0, lf_nw = 0;
    size_t recon_lds = 0, lf_lds = 0;
    vp8hip_stats stats = {};
    // Small launches spread every frame pair over several CUs (vp8_recon_xcu_kernel / vp8_loopfilter_xcu_kernel): granule
    // buffers of the row-to-row hand-over (capacities in bytes), the launch counter that tags the granules, and the status word a
    // kernel sets (host-mapped memory) when a hand-over does not arrive
    DevBuf<unsigned long long> gran_recon, gran_lf;
    unsigned int epoch = 0;
    MappedBuf<int> h_status; int *d_status = nullptr;
    DevBuf<uint8_t> d_i420; Event ev_pack;           // vp8hip_frames_fetch_i420_async: the batch as packed I420, before it leaves (capacity in bytes, 256 more are there)
    DevBuf<uint8_t> d_rgb;                           // vp8hip_frames_rgb_async: a chunk of frames as packed I420 at the scaled size (a cache)
    Event ev_d2h_more[3];                            // the piece on stream_d2h_more[k] has left
    Event ev_d2h_from, ev_d2h_done;
    int d2h_first = 0, d2h_count = 0;  // frame buffers of the copy in flight (count 0: none)
    std::vector<uint8_t> d2h_mask; bool d2h_listed = false;     // ... of a fetch by list (vp8hip_frames_md5_list_async): a flag per frame buffer
    DevBuf<uint8_t> d_md5;         // vp8hip_frames_fetch_async: the batch's digests on the device (capacity in digests)
    DevBuf<int> d_md5_idx; PinnedBuf<int> h_md5_idx;    // vp8hip_frames_md5_list_async: which frame buffers
    size_t fb_stride = 0;
    DevBuf<unsigned int> d_intra_flags;              // per job of a launch: the frame has intra macroblocks (vp8_inter_mb_kernel)
    // vp8hip_postproc: dither table (440 shorts), noise table (3072) and per-row noise phases (16384) on the device
    DevBuf<char> d_pp; PinnedBuf<char> h_pp; bool pp_rv_loaded = false; Event ev_pp;
    DevBuf<uint8_t> d_mfqe; PinnedBuf<uint8_t> h_mfqe; Event ev_mfqe;     // vp8hip_mfqe: the macroblock classes of the frame
    DevBuf<char> d_vis; PinnedBuf<char> h_vis; Event ev_vis;         // vp8hip_visualize: the frame-info and rate strings on their way to the device
    // vp8hip_entropy_decode: the frames' descriptions, their bytes, per-frame scratch and status on the device; the stream the
    // launch's input is copied on (stream_h2d: beside the pixel path of other slots) and the events that order it against the main
    // stream (descriptions and bytes in TWO sets, capacities in bytes: a launch's input is copied while the launch before
    // and its frames' pixel path still run -- 3 to 5 GB per launch of 24,576 1080p frames; ev_ent_in[k]: set k's copies have landed,
    // ev_ent_out[k]: the kernel that read set k is done)
    DevBuf<char> d_ent_frames2[2]; DevBuf<uint8_t> d_ent_data2[2]; int ent_set = 0;
    Event ev_ent_in[2], ev_ent_out[2];
    DevBuf<unsigned int> d_ent_scratch, d_ent_status; int ent_last_count = 0;
    struct { int count = 0, set = 0, np = 0; const vp8hip_entropy_frame *frames = nullptr; size_t data_bytes = 0; } ent_staged;    // input sent, kernel not yet launched (count 0: none)
    bool ent_tables_loaded = false, ent_parts_off = false; int ent_lpw = 0;
    int ent_resident[3] = {};      // waves of vp8_entropy_kernel the device holds at once with 64 / 32 / 16 lanes carrying a frame (LDS)
    DevBuf<unsigned int> d_sched;  // vp8_keyframe_kernel's role / work counters
    DevBuf<unsigned short> d_subpel_cost;            // vp8hip_frames_subpel_async: the cost table of the call (SUBPEL_TABLE_ENTRIES, made with the first table)
};

int vp8hip_fail(vp8hip_ctx *c, int code, const char *fmt, ...);
#define fail vp8hip_fail
#define HIPCHK(ctx, call)                                                                          \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess) return fail(ctx, -1, "%s failed: %s", #call, hipGetErrorString(e_)); \
    } while (0)

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

#define FB_RASTER 1u            // fb_state bits: the raster form holds the frame (borders included) ...
#define FB_TILES  2u            // ... the tiled form does
// vp8hip_launch.hip: make sure the raster form of frame buffers first .. first + count - 1 holds their frames (a tiled -> raster
// pass + border extension on the context's stream for those that are only there as tiles)
// The raster pool itself is allocated when something first needs it (vp8hip_raster_pool; c->fb[i] are null until then): a
// pipeline whose frames are written as tiles, hashed as tiles and never read by coordinate never pays for it -- at 1080p 3.2 MB
// per frame buffer, a quarter of what a frame in flight costs.
int vp8hip_raster_pool(vp8hip_ctx *c);
int vp8hip_drop_staging(vp8hip_ctx *c);       // vp8hip.hip: frees the packed staging and the RGB call's scratch (1: freed, 0: there was none)
int vp8hip_need_raster(vp8hip_ctx *c, int first, int count);
int vp8hip_need_raster_list(vp8hip_ctx *c, const int *fbs, int n);
// vp8hip.hip
int vp8hip_check_status(vp8hip_ctx *c);       // after a stream synchronisation: did a kernel of the cross-CU family give up on a hand-over?
// vp8hip_scale.hip: what vp8hip_frames_scale_async and vp8hip_frames_rgb_async (vp8hip_rgb.hip) share -- the plan of a target size
// (returns the LDS a workgroup takes), one launch of at most SCALE_MAX_FRAMES frames
int vp8hip_scale_plan(const vp8hip_ctx *c, int dw, int dh, int filter, ScaleLaunch &L);
int vp8hip_scale_enqueue(vp8hip_ctx *c, const int *fbs, int m, ScaleLaunch &L, int lds, void *dst, size_t dst_stride);
// vp8hip_rgb.hip: the conversion's coefficients by position, for the kernels that make RGB bytes (vp8_rgb.hip, vp8_trace_residual.hip)
void vp8hip_rgb_coeffs(int matrix, int order, int &cy, int &k0, int (&cu)[3], int (&cv)[3]);
// the form a reader that converts nothing takes a frame buffer in: raster where it exists, else tiles; never written: zeros
static inline int vp8hip_frame_form(const vp8hip_ctx *c, int fb)
{
    const uint8_t st = c->fb_state[(size_t)fb];
    return (st & FB_RASTER) && c->fb_block ? SCALE_FROM_RASTER : (st & FB_TILES) ? SCALE_FROM_TILES : SCALE_FROM_ZERO;
}
// ... and how a launch names it to such a reader: frame buffer << 2 | that form, as of the call (the frame buffers of a job each
// in a form of their own)
static inline int vp8hip_frame_ref(const vp8hip_ctx *c, int fb) { return fb << 2 | vp8hip_frame_form(c, fb); }

// vp8hip_handover.hip: what the calls that write tensors into the caller's device memory share.  The checks return 0, or -2
// with the error set (its text begins with `who`); vp8hip_check_dst: stride >= size, destination and stride aligned to the
// element, then vp8hip_check_device_span: device memory of the context's device, the n frames inside one allocation;
// vp8hip_check_named_dst: the same for a call of several destinations, its texts begun with "`who` (`name`)".
// vp8hip_check_pairs: fb, then ref_fb of each of n picture pairs (ref_optional: a ref_fb of exactly -1 names none);
// vp8hip_frame_planes: where the planes of the context's frame buffers lie, for the kernels that read such pairs.
#define VP8HIP_MAX_OUT_SIZE 16383       // the largest width / height of an output
#define VP8HIP_GATHER_MAX_CHANNELS 4096 // the most channels of a tensor vp8hip_trace_gather_async moves
#define VP8HIP_HIST_YUV (VP8HIP_HIST_Y | VP8HIP_HIST_U | VP8HIP_HIST_V)
int vp8hip_check_fbs(vp8hip_ctx *c, const char *who, const int *fbs, int n);
int vp8hip_check_pairs(vp8hip_ctx *c, const char *who, const vp8hip_hist_job *jobs, int n, bool ref_optional);
void vp8hip_frame_planes(const vp8hip_ctx *c, FramePlanes &L);
int vp8hip_check_named_dst(vp8hip_ctx *c, const char *who, const char *name, const void *dst, size_t dst_stride, size_t size, size_t elem_size, int n);
int vp8hip_check_slots(vp8hip_ctx *c, const char *who, const int *slots, int n);
// vp8hip_quant.hip: what vp8hip_frames_quant_async and vp8hip_frames_intra_async share of a vp8hip_quant -- the check of its quantiser
// part, and table k of a launch: vp8hip_quant_factors for qindex as it stands, then the three ZBIN_EXTRAs (QUANT_TABLE_SHORTS shorts)
#define QUANT_ZBIN_MAX (1 << 20)
bool vp8hip_quantiser_ok(const vp8hip_quant *p);
void vp8hip_quant_staged_table(short *t, int qindex, const vp8hip_quant *p);
bool vp8hip_out_grid(const vp8hip_ctx *c, int dst_w, int dst_h, int cells, int &gw, int &gh);
int vp8hip_check_device_span(vp8hip_ctx *c, const char *who, const void *dst, size_t dst_stride, size_t size, int n);
int vp8hip_check_dst(vp8hip_ctx *c, const char *who, const void *dst, size_t dst_stride, size_t size, size_t elem_size, int n);
unsigned vp8hip_segment_q_bits(const vp8ir_frame_hdr &h);
// vp8hip_side.hip: what the kernels that read a slot's records take of its header (SideLaunch::q, HistSlotLaunch::q): vp8hip_segment_q_bits,
// and bit 28 for a key frame
unsigned vp8hip_side_header_bits(const vp8ir_frame_hdr &h);
// vp8hip_residual.hip: what the kernels that dequantise take of a slot's header (ResLaunch::s, CoefLaunch::s): the quantiser index
// of each segment and the five *_delta_q
ResSlot vp8hip_res_header_bits(int slot, const vp8ir_frame_hdr &h);
// vp8hip_trace.hip, for the calls that read a pool in the caller's device memory (those there and vp8hip_hist.hip): a pool of
// pool_frames entries of the context's trace size, pool_stride apart, dword-aligned, inside one allocation of the device; and
// whether [p, + stride * frames) and [q, + qstride * qframes) overlap
int vp8hip_check_pool(vp8hip_ctx *c, const char *who, const void *pool, size_t pool_stride, int pool_frames);
bool vp8hip_spans_overlap(const void *p, size_t stride, int frames, const void *q, size_t qstride, int qframes);
// bytes of an element by dtype: F16 is 1 and F32 is 2 in VP8HIP_RGB_*, VP8HIP_SIDE_* and VP8HIP_RES_*; size0: type 0's (bytes: 1, int16: 2)
static inline int vp8hip_elem_size(int dtype, int size0) { return dtype == 2 ? 4 : dtype == 1 ? 2 : size0; }
