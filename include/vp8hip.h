/* include/vp8hip.h -- C ABI of the MI355X (gfx950) VP8 pixel path: libvp8hip.so.
 *
 * Plain C, opaque handle, int status returns (0 = OK, negative = error; text via
 * vp8hip_last_error), no HIP / C++ / torch types in any signature.  This is the frame-granular
 * boundary that sits where the reference's OpenCL offload branches sit (SURVEY.md 8b "B3"):
 *
 *   vp8hip_create / vp8hip_destroy      <- vp8dx_create_decompressor / vp8dx_remove_decompressor
 *                                          (vp8/decoder/onyxd_if.c:73,136) + cl_init/cl_destroy
 *                                          (vp8/common/opencl/vp8_opencl.c:40-84,155-260)
 *   vp8hip_configure                    <- vp8_alloc_frame_buffers (vp8/common/alloccommon.c:59)
 *                                          incl. the per-frame-buffer device memory the reference
 *                                          attaches as YV12_BUFFER_CONFIG.buffer_mem
 *                                          (vpx_scale/yv12config.h:63-65, yv12config.c:97-105)
 *   vp8hip_ir_map_compact /             <- the per-MB submit points of the reference's CL path
 *   vp8hip_ir_upload_compact               (vp8/decoder/decodframe.c:149-156: qcoeff/eobs/MODE_INFO
 *   (vp8hip_ir_map / vp8hip_ir_upload:     handed to vp8_decode_macroblock_cl)
 *    the same from dense arrays)
 *   vp8hip_decode                       <- decode_mb_row x mb_rows (decodframe.c:1116-1129),
 *                                          vp8_loop_filter_frame (vp8/common/loopfilter.c:203; its
 *                                          CL diversion at :225-230) and
 *                                          vp8_yv12_extend_frame_borders_ptr (onyxd_if.c:607)
 *   vp8hip_frame_download               <- the read-back of loopfilter_cl.c:688-696 / the plane
 *                                          pointers vp8dx_get_raw_frame exposes (onyxd_if.c:707)
 *
 * There is NO CPU fallback behind this interface: if the GPU or the code object is unavailable
 * vp8hip_create fails and the decoder built on it reports VPX_CODEC_ERROR.
 *
 * Threading: one context per decoder / per GPU; a context is not thread-safe.
 */
#ifndef VP8HIP_H
#define VP8HIP_H

#include <stddef.h>
#include <stdint.h>
#include "vp8_ir.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vp8hip_ctx vp8hip_ctx;

#define VP8HIP_STAGE_RECON   1   /* dequant+IDCT/WHT, intra + inter prediction, add            */
#define VP8HIP_STAGE_LF      2   /* in-loop deblocking (no-op for frames with filter_level 0) */
#define VP8HIP_STAGE_EXTEND  4   /* 32/16-px border replication                               */
#define VP8HIP_STAGE_ALL     7

/* One frame of work.  Slots and frame buffers are indices into the pools sized by
 * vp8hip_configure.  ref_fb[VP8IR_LAST_FRAME..VP8IR_ALTREF_FRAME] are read by inter MBs only
 * (ref_fb[0] unused; -1 where a reference does not exist).  Jobs passed to ONE vp8hip_decode
 * call must be mutually independent (no job's dst_fb is another's ref_fb): they run concurrently. */
typedef struct vp8hip_job {
    int32_t ir_slot;
    int32_t dst_fb;
    int32_t ref_fb[4];
} vp8hip_job;

typedef struct vp8hip_stats {      /* filled by vp8hip_get_stats; times from HIP events, ms */
    float recon_ms, lf_ms, extend_ms;   /* last vp8hip_decode call; extend_ms = border extension (wave-per-row kernels), or the
                                           tiled -> raster pass + borders if the launch ran it at once (detile_pass) */
    int   recon_waves, lf_waves;        /* waves per workgroup (1 = the lane-per-row kernels ran, 4 = the cross-CU
                                           variant of the wave-per-row kernels: small launches) */
    int   workgroups;
    int   detile_pass;                  /* 1: the launch produced the raster form of its frames at once (VP8HIP_EAGER_RASTER); by
                                           default a large launch leaves tiles and the pass runs when the raster form is asked for */
    int   lf_kernels;                   /* loop-filter kernels launched: 1 (wave-per-row family, some frame filtered) or 0 */
    int   fused;                        /* 1: the lane-per-row kernels -- vp8_keyframe_kernel, or vp8_inter_pred_kernel +
                                           vp8_interframe_kernel -- reconstructed AND filtered the launch; recon_ms covers it,
                                           lf_ms is 0 */
    int   pred_tiles;                   /* 1: the launch predicted its inter macroblocks from reference frames read as TILES
                                           (vp8_inter_pred_tiles_kernel: what the launch before left, no tiled -> raster pass in
                                           between); 0: from their border-extended raster form */
} vp8hip_stats;

/* device < 0: use the current HIP device.  Returns 0 or a negative error. */
int  vp8hip_create(int device, vp8hip_ctx **out);
void vp8hip_destroy(vp8hip_ctx *ctx);
const char *vp8hip_last_error(const vp8hip_ctx *ctx);   /* ctx may be NULL: creation error */

/* (Re)allocate device state for frames of width x height: num_fb frame buffers (vp8ir_geom layout, borders included) and
 * num_slots IR slots.  A slot holds one frame's macroblock data in the DEVICE FORM of include/vp8_ir.h (records, block stream
 * sized for the worst case, vectors: 960 bytes per macroblock) and gets pinned host staging of the same layout when it is first
 * mapped.  Existing contents are discarded, and so is input staged by vp8hip_entropy_stage and not launched (once its copy has
 * finished reading the caller's memory). */
int  vp8hip_configure(vp8hip_ctx *ctx, int width, int height, int num_fb, int num_slots);
/* The same with the slots' block streams out of ONE pool.  The worst case a slot of vp8hip_configure is sized for -- 24 blocks a
 * macroblock, 768 of its 960 bytes per macroblock -- is rarely what a frame needs (a 1080p key frame of 200 KB: 62 k blocks = 2.0 of
 * 6.3 MB), and frames in flight are what the device's entropy decoder lives on (vp8hip_entropy_decode: a frame per lane).  Here a
 * slot holds records and vectors only (192 bytes per macroblock) and the entropy decoder takes the blocks' room out of the pool as
 * it goes, a chunk (four macroblock rows' worst case) at a time: a row's blocks stay together, the records' sparse_first count
 * from the pool's start, and vp8hip_decode reads the slots as ever.  vp8hip_pool_reset (on the context's stream: after the launches
 * queued so far) empties the pool -- when the frames decoded out of it have been through vp8hip_decode; the caller says when.  A
 * frame that finds the pool empty gets bit 1 of its status word (vp8hip_entropy_status) and is not to be decoded for its pixels: the
 * blocks it could not place went into the spare chunk behind the pool's last (all such frames share it), so its records'
 * sparse_first still point INSIDE the pool's allocation -- a vp8hip_decode over such a slot, queued before the status has come back,
 * reads and writes nothing out of bounds; what it leaves in the frame buffer is garbage (tests/test_gpu_entropy.py).  The host-side
 * producers (vp8hip_ir_map*, vp8hip_ir_upload*) are refused on such a context; vp8hip_ir_copy copies the records, which then share
 * the blocks; frames with several token partitions are decoded a frame per lane.  vp8hip_pool_usage (synchronises): bytes taken
 * since the last reset (more than *pool_bytes: that much was asked for) and the pool's size. */
int  vp8hip_configure_pooled(vp8hip_ctx *ctx, int width, int height, int num_fb, int num_slots, size_t pool_bytes);
int  vp8hip_pool_reset(vp8hip_ctx *ctx);
int  vp8hip_pool_usage(vp8hip_ctx *ctx, size_t *used_bytes, size_t *pool_bytes);
/* The two forms' pools are allocated when a launch or a reader first needs them (the tiled forms with the first large launch, the
 * raster forms with the first small launch, inter frame, download or filter); vp8hip_reserve allocates them now -- beside a first
 * launch of the entropy decoder, for instance: tens of GB take the allocator a second or two. */
int  vp8hip_reserve(vp8hip_ctx *ctx, int tiled_form, int raster_form);
/* What the context holds on the device right now, in bytes: the raster forms' pool, the tiled forms' pool, the IR slots, the block
 * pool (vp8hip_configure_pooled), the entropy decoder's input buffers, the staging of packed downloads. */
typedef struct vp8hip_memory {
    size_t raster_pool, tile_pool, slots, block_pool, entropy_input, packed_staging;
} vp8hip_memory;
int  vp8hip_memory_usage(const vp8hip_ctx *ctx, vp8hip_memory *out);
/* packed_staging: the batch as packed I420 -- what vp8hip_frames_fetch_i420_async sends, and what a digest-only fetch of
 * VP8HIP_MD5_PACK_FROM (12,288) tiled frames and more is hashed from: 3.1 MB per 1080p frame, 51 GB at 16,384, allocated when first
 * needed (a fetch that finds no room for it hashes the tiles) and KEPT for the next batch.  It is a cache: the library frees it by
 * itself when one of the two pools cannot be allocated beside it, and vp8hip_release_staging frees it now (waits for fetches in
 * flight).  The scratch of vp8hip_frames_rgb_async (scaled frames as packed I420, at most 256 MB; vp8hip_rgb_scratch_bytes, not one
 * of the six fields) is a cache of the same kind and is freed by the same call. */
int  vp8hip_release_staging(vp8hip_ctx *ctx);
int  vp8hip_geometry(const vp8hip_ctx *ctx, vp8ir_geom *g);

/* Pinned host staging of a slot in the device form, for a feeder to write into directly (vp8_parser_decode_mbs_compact): mbx[nmb],
 * blocks[*cap_blocks * 16] right behind them, mvs[nmb * 16].  vp8hip_ir_upload_compact sends header, records and the first
 * nblocks blocks with ONE asynchronous copy on the context's stream (+ one for the vectors of an inter frame); the pixel
 * kernels read what arrives, nothing on the device touches it in between.  The staging may be rewritten once that copy has run
 * (vp8hip_sync, or any later synchronisation of the stream). */
int  vp8hip_ir_map_compact(vp8hip_ctx *ctx, int slot, vp8ir_frame_hdr **hdr, vp8ir_mbx **mbx, int16_t **blocks, size_t *cap_blocks,
                           vp8ir_mv **mvs);
int  vp8hip_ir_upload_compact(vp8hip_ctx *ctx, int slot, size_t nblocks);
/* The same from the DENSE view (mbs[nmb], coef[nmb * 400]: what the oracle and the tests speak): host memory the caller fills;
 * vp8hip_ir_upload turns it into the device form on the host (vp8ir_compact_mb), in the slot's staging, and uploads that.  It
 * waits for the context's stream first (the staging may still be on its way from the upload before). */
int  vp8hip_ir_map(vp8hip_ctx *ctx, int slot, vp8ir_frame_hdr **hdr, vp8ir_mb **mbs,
                   int16_t **coef, vp8ir_mv **mvs);
int  vp8hip_ir_upload(vp8hip_ctx *ctx, int slot);
/* Device-to-device replication of a slot (synthetic looped streams: every key frame
 * is independently decodable, decodframe.c:610-639). */
int  vp8hip_ir_copy(vp8hip_ctx *ctx, int dst_slot, int src_slot);

/* Enqueue the pixel path for njobs independent frames on the context's stream.  `stages` is a
 * mask of VP8HIP_STAGE_*.  Asynchronous; see vp8hip_sync. */
int  vp8hip_decode(vp8hip_ctx *ctx, const vp8hip_job *jobs, int njobs, int stages);

/* Copy one frame buffer to the host.  full != 0: the whole buffer (frame_size bytes, borders
 * included) into y (u, v ignored).  Otherwise the visible planes: rows of width x height (Y) and
 * ((w+1)/2) x ((h+1)/2) (U, V) written with the given destination strides.  Synchronous. */
int  vp8hip_frame_download(vp8hip_ctx *ctx, int fb, int full, uint8_t *y, uint8_t *u, uint8_t *v,
                           int y_stride, int uv_stride);
/* Output-side post-processing (vp8/common/postproc.c): frame buffer src_fb -> dst_fb, never back into
 * decoding.  The policy stays with the caller, as in the reference where vp8_post_proc_frame (postproc.c:903-1000) sits above
 * the filters: it turns the frame's loop-filter level into the thresholds and draws the random phases.
 *   VP8HIP_PP_DEBLOCK       vp8_deblock (:348-362): vp8_post_proc_down_and_across on Y, U, V with `flimit`
 *   VP8HIP_PP_DEMACROBLOCK  vp8_deblock_and_de_macro_block (:328-346): the same, then vp8_mbpost_proc_across_ip and
 *                           vp8_mbpost_proc_down on Y with `mb_flimit`; needs tmp_fb (a third buffer) and the dither table
 *                           `rv` (vp8_rv, 440 entries) with this frame's rv_offset = 63 & rand() (:286)
 *   VP8HIP_PP_ADDNOISE      vp8_plane_add_noise (:489-513) on Y: `noise` = the 3072-entry table fillrd (:410-465) built (NULL:
 *                           unchanged since the previous call), noise_clamp = its blackclamp[0], noise_rows[r] = rand() & 0xff
 *                           per row of the 16-aligned height.  Frames wider than 2816 are refused: the reference indexes
 *                           past the end of its table for them.
 * With neither of the first two flags dst_fb becomes a copy of src_fb (:982), or, with dst_fb == src_fb, stays what it is (the
 * noise alone, in place: after vp8hip_mfqe).  The filters read nothing outside the pictures' coded area (rows above and below
 * are the edge rows, as a frame's borders would say).  Asynchronous on the context's stream like
 * vp8hip_decode; the host arrays may be reused when the call returns. */
#define VP8HIP_PP_DEBLOCK       1
#define VP8HIP_PP_DEMACROBLOCK  2
#define VP8HIP_PP_ADDNOISE      4
typedef struct vp8hip_pp {
    int32_t flags;
    int32_t flimit;
    int32_t mb_flimit;
    int32_t rv_offset;
    int32_t noise_clamp;
    const int16_t *rv;
    const int8_t  *noise;
    const uint8_t *noise_rows;
} vp8hip_pp;
int  vp8hip_postproc(vp8hip_ctx *ctx, int src_fb, int dst_fb, int tmp_fb, const vp8hip_pp *pp);
/* VP8_MFQE, vp8_multiframe_quality_enhance (postproc.c:802-900): the frame about to be shown (show_fb) against the picture that
 * was shown before it (prev_fb: the output of the previous call chain, noise and all), macroblock by macroblock -- where the two
 * differ little for the old picture's activity and the step from qprev to qcurr the old picture is kept or blended in (it was
 * coded with the finer quantiser), elsewhere the new one is copied -- into dst_fb, which may be prev_fb.  mb_class: a byte per
 * macroblock in raster order, 0 = copy (inter frame, a vector component above 10: :836-841), 1 = one 16x16 block, 2 = four 8x8
 * blocks (B_PRED, SPLITMV: :843).  When to call it is the caller's policy, as for the filters (vp8_post_proc_frame :948-969:
 * from the second shown frame on, when base_qindex is 10 or more above the running last_base_qindex; the filters then run on
 * its output: vp8hip_postproc(dst_fb -> prev_fb), or with src_fb == dst_fb for the noise alone).  qprev <= qcurr <= 127.
 * Asynchronous on the context's stream; mb_class may be reused when the call returns. */
int  vp8hip_mfqe(vp8hip_ctx *ctx, int show_fb, int prev_fb, int dst_fb, const uint8_t *mb_class, int qcurr, int qprev);
/* The decoder's debug overlays (vp8/common/postproc.c:1007-1362, CONFIG_POSTPROC_VISUALIZER) drawn into frame buffer fb in place,
 * from the macroblocks of IR slot ir_slot (modes, reference frames, sub-block modes, skip flags; the vectors of an inter frame),
 * in the reference's order: the text the VP8HIP_VIS_TXT_* flags ask for (7x5 characters of 0 / 255 addressed linearly from the
 * luma origin: a long string runs on into the rows below), the motion vectors of the modes in mv_mask as inverted Bresenham
 * lines, the block-mode colours (mb_modes_mask: macroblock modes, where the VALUE 4 also selects B_PRED's sub-blocks; b_modes_mask:
 * sub-blocks of B_PRED macroblocks when it has bit B_PRED), the reference-frame colours of the frames in ref_frame_mask.  The
 * flags are the VP8D_DEBUG_* bits of vp8/common/ppflags.h; a phase runs when its flag and its mask are set, the masks are the
 * values of the VP8_SET_DBG_* controls.  The strings are formatted by the caller (NULL: not drawn), at most 511 characters.
 * Writes that would leave the frame buffer are dropped.  Asynchronous on the context's stream; the strings may be reused when the
 * call returns. */
#define VP8HIP_VIS_TXT_FRAME_INFO     (1u << 3)
#define VP8HIP_VIS_TXT_MBLK_MODES     (1u << 4)
#define VP8HIP_VIS_TXT_DC_DIFF        (1u << 5)
#define VP8HIP_VIS_TXT_RATE_INFO      (1u << 6)
#define VP8HIP_VIS_DRAW_MV            (1u << 7)
#define VP8HIP_VIS_CLR_BLK_MODES      (1u << 8)
#define VP8HIP_VIS_CLR_FRM_REF_BLKS   (1u << 9)
typedef struct vp8hip_vis {
    unsigned flags;           /* VP8HIP_VIS_* (VP8D_DEBUG_*) bits; others are ignored */
    int ref_frame_mask, mb_modes_mask, b_modes_mask, mv_mask;   /* the four VP8_SET_DBG_* values */
    const char *frame_info;   /* host-formatted, or NULL */
    const char *rate_info;    /* host-formatted, or NULL */
} vp8hip_vis;
int  vp8hip_visualize(vp8hip_ctx *ctx, int fb, int ir_slot, const vp8hip_vis *v);

/* Entropy decoding on the device (key frames).  What it replaces: the per-macroblock half of the host feeder -- the reference's
 * vp8_kfread_modes (vp8/decoder/decodemv.c:50-173) and vp8_decode_mb_tokens (vp8/decoder/detokenize.c:183-405) driven by
 * decode_mb_row (vp8/decoder/decodframe.c:293-470) -- which at ~10 ms per 1080p frame and core is what bounds a pipeline that
 * starts from the compressed stream.  A bool decoder is a serial machine, so a frame is ONE LANE's work (its token partitions
 * decoded in macroblock-row order like the reference's single thread does); the frames of a batch run side by side, 64 to a
 * wave.  The frame header stays with the host (a few thousand bools: vp8_parser_begin_frame), which hands over what it leaves
 * behind (vp8_parser_export_entropy, csrc/host/vp8_parser.h): the decoder state of the first partition where the per-macroblock
 * data start, the token partitions' extents, the probabilities.  The kernel writes the frames' slots in the device form of
 * include/vp8_ir.h -- what vp8_parser_decode_mbs_compact writes on the host -- and vp8hip_decode reads it as it stands.  Inter
 * frames too (vp8_decode_mode_mvs' per-macroblock half: reference frame, the near / nearest candidates from the
 * macroblocks above, left and above-left, NEWMV / SPLITMV vectors: decodemv.c:323-569) -- which only pays where many frames are
 * independent of each other, as the same position of many streams is.  Integer only. */
typedef struct vp8hip_entropy_frame {
    vp8ir_frame_hdr hdr;                /* as vp8_parser_begin_frame returned it; a frame of the context's size */
    uint64_t data_off;                  /* the frame's first byte in the buffer handed to vp8hip_entropy_decode */
    uint32_t first_pos, first_end;      /* first partition, relative to data_off: the next byte the decoder takes, and its end */
    uint32_t first_value;               /* ... its window (32 bits, the active byte on top), */
    int32_t  first_bits;                /*     the valid bits below the top byte (negative: refill due), */
    uint32_t first_range;               /*     and its range, 128..255 */
    uint32_t num_tok;                   /* 1, 2, 4 or 8 token partitions */
    uint32_t tok_pos[8], tok_end[8];    /* their extents, relative to data_off */
    uint8_t  update_mb_segmentation_map, mb_no_coeff_skip, prob_skip_false;
    uint8_t  segmap_keep;               /* 1: a macroblock's segment id is the one the slot's record holds from the frame before
                                           (a stream decoded frame after frame into this slot: vp8_parser_set_device_segmap) */
    uint8_t  segment_tree_probs[3], rsv1;
    uint8_t  coef_probs[1056];          /* [block type 4][band 8][context 3][node 11] */
    /* inter frames (hdr.frame_type 1; mb_mode_mv_init, decodemv.c:178-224): */
    uint8_t  prob_intra, prob_last, prob_gf, rsv2;
    uint8_t  ymode_prob[4];
    uint8_t  uvmode_prob[3], rsv3;
    uint8_t  mvc[2][19], rsv4[2];       /* motion-vector probabilities, row then column */
    uint8_t  rsv5[4];
} vp8hip_entropy_frame;
/* frames[i] -> IR slot first_slot + i.  `data`: the compressed frames (data_bytes in all; any host memory -- page-locked memory
 * from vp8hip_host_alloc makes the copy asynchronous, and then `frames` and `data` have to stay untouched until the next
 * vp8hip_sync).  Asynchronous on the context's stream. */
int  vp8hip_entropy_decode(vp8hip_ctx *ctx, int first_slot, int count, const vp8hip_entropy_frame *frames, const uint8_t *data,
                           size_t data_bytes);
/* The same in two steps, for a pipeline that wants the NEXT launch's input on its way while it still queues and waits on behalf of
 * the current one: vp8hip_entropy_stage checks the frames and sends them to the device (its own copy stream, one of two buffers),
 * vp8hip_entropy_decode(ctx, first_slot, count, NULL, NULL, 0) launches the kernel over what was staged.  One staged input at a time. */
int  vp8hip_entropy_stage(vp8hip_ctx *ctx, int count, const vp8hip_entropy_frame *frames, const uint8_t *data, size_t data_bytes);
/* What became of the frames of the last vp8hip_entropy_decode, a word each: bit 1 = the block pool was empty (vp8hip_configure_pooled:
 * the frame's slot is not to be decoded); bit 0 = a partition of the frame ended early, the
 * frame is corrupt (what vp8_parser_decode_mbs reports through *corrupt).  Synchronous.  _async: the copy is queued on the
 * context's stream into page-locked memory of the caller's (vp8hip_host_alloc) and has landed after the next synchronisation
 * (vp8hip_sync, or vp8hip_download_wait for a fetch queued behind it). */
int  vp8hip_entropy_status(vp8hip_ctx *ctx, int count, uint32_t *status);
int  vp8hip_entropy_status_async(vp8hip_ctx *ctx, int count, uint32_t *status);
/* The IR of a slot as it stands on the device, expanded to the dense view on the host (tests, debugging): mbs[nmb],
 * coef[nmb * 400], zeros where a block has no coefficients.  Synchronous. */
int  vp8hip_ir_fetch(vp8hip_ctx *ctx, int slot, vp8ir_mb *mbs, int16_t *coef);
int  vp8hip_ir_fetch_mvs(vp8hip_ctx *ctx, int slot, vp8ir_mv *mvs);      /* ... and its vectors: mvs[nmb * 16] */

/* Batch form for pipelines (tools/e2e.py, bin/batch_md5): `count` consecutive frame buffers, whole, as ONE asynchronous copy on
 * a stream of its own -- it starts when everything queued on the context's stream so far has finished and runs beside later
 * uploads (PCIe is full duplex).  dst: page-locked memory (vp8hip_host_alloc), frame i at dst + i * vp8hip_frame_stride(ctx)
 * (frame_size rounded up to 256).  vp8hip_download_wait returns when the copy has landed; one copy in flight at a time; a
 * launch that writes one of these frame buffers waits for it by itself. */
size_t vp8hip_frame_stride(const vp8hip_ctx *ctx);
int  vp8hip_frames_download_async(vp8hip_ctx *ctx, int first_fb, int count, uint8_t *dst);
int  vp8hip_download_wait(vp8hip_ctx *ctx);
/* The same with the frames' MD5s computed on the device: what `vpxdec --md5` (vpxdec.c:1080-1101) and examples/decode_to_md5
 * (decode_to_md5.txt) hash on the host -- the visible rows of the Y, U and V planes, vpx_image_t d_w x d_h -- one 16-byte digest
 * per frame into digests[16 * i], a frame per lane (csrc/hip/vp8_md5.hip).  dst and digests may each be NULL (not both); both
 * have landed when vp8hip_download_wait returns.  Any display size: where a row is whole MD5 blocks (width a multiple of 128) the
 * kernel reads block by block, from whichever form the frames are in; other widths are hashed from the raster form by a kernel
 * whose blocks straddle rows (correct, slower: the conformance streams' odd sizes, not the throughput path). */
int  vp8hip_frames_fetch_async(vp8hip_ctx *ctx, int first_fb, int count, uint8_t *dst, uint8_t *digests);
/* The same with the frames delivered as PACKED I420: d_w x d_h luma, then the two (d_w / 2) x ((d_h + 1) / 2) chroma planes, back to
 * back, no borders, no strides -- what `vpxdec --i420` writes (vpxdec.c:1080-1101) and what the digests are taken over --,
 * vp8hip_i420_bytes() per frame, frame i at dst + i * vp8hip_i420_bytes().  A pass on the device packs the frames from whichever
 * form they are in (tiles as they are; no raster form is needed), the copy engines take them out: a tenth less over the link than
 * whole frame buffers (1080p: 3.11 MB a frame instead of 3.43), which is what a pipeline that downloads every frame is bound by.
 * Display widths that are not a multiple of 8 are refused with -3. */
size_t vp8hip_i420_bytes(const vp8hip_ctx *ctx);
int  vp8hip_frames_fetch_i420_async(vp8hip_ctx *ctx, int first_fb, int count, uint8_t *dst, uint8_t *digests);
/* The digests alone, of ANY n frame buffers (fbs[i]; not necessarily neighbours: the shown frames of many streams decoded side by
 * side, bin/batch_md5 --streams): digests[16 * i].  Same stream and same wait as vp8hip_frames_fetch_async. */
int  vp8hip_frames_md5_list_async(vp8hip_ctx *ctx, const int *fbs, int n, uint8_t *digests);
/* Frames for consumers on the device       <- I420Scale, third_party/libyuv/source/scale.c:3762
 * Any n frame buffers (fbs: any order, repeats allowed; reusable when the call returns) as PACKED I420 in the caller's DEVICE
 * memory: dst_w x dst_h luma, then U and V, each ((dst_w + 1) / 2) x ((dst_h + 1) / 2), no padding, vp8hip_i420_size(dst_w,
 * dst_h) bytes; frame i at dst + i * dst_stride, any byte alignment.  At the display size the call is a plain copy (any width);
 * otherwise the bytes are those of the reference tree's libyuv (its C rows) scaling the image vpx_codec_get_frame returns:
 * filter 0 point sampling, 1 bilinear, 2 (kFilterBox) the same as 1 -- I420Scale never reaches its box filter.  Each frame is
 * read in a form it has (raster where it exists, else tiles): nothing is converted or allocated.  Enqueued on the context's
 * stream (vp8hip_stream): later launches that write these frame buffers run behind it; a caller's stream waits on it with an
 * event.  Only bytes inside [dst + i * dst_stride, + size) are written.  Returns -2, with nothing enqueued, for n < 1, a frame
 * buffer out of range, a size outside 1..16383, another filter, dst_stride < size, a dst that is not device memory of the
 * context's device, or n frames that do not fit in dst's allocation.  vp8hip_i420_size: 0 outside 1..16383. */
size_t vp8hip_i420_size(int w, int h);
int  vp8hip_frames_scale_async(vp8hip_ctx *ctx, const int *fbs, int n, int dst_w, int dst_h, int filter, void *dst, size_t dst_stride);
/* Frames for models on the device: RGB tensors (bytes, halves or floats)
 * The result for a frame is convert(S), S being the packed I420 image vp8hip_frames_scale_async would write for the same
 * (frame buffer, dst_w, dst_h, filter): sizes, libyuv's paths, odd sizes and the clamp to the aligned area are the scaler's, bit
 * for bit.  convert, for output pixel (x, y): Y = S.y[y][x], U = S.u[y >> 1][x >> 1], V = S.v[y >> 1][x >> 1] (chroma replicated,
 * not interpolated), then in 32-bit integers, >> arithmetic:
 *     l = cy * (Y - yoff) + 128
 *     R = clamp255((l + crv * (V - 128)) >> 8)
 *     G = clamp255((l + cgu * (U - 128) + cgv * (V - 128)) >> 8)
 *     B = clamp255((l + cbu * (U - 128)) >> 8)
 *     matrix                            yoff   cy  crv   cgu   cgv  cbu      (the exact matrices times 256, rounded: within 1 of
 *     VP8HIP_RGB_BT601 (limited range)    16  298  409  -100  -208  516       the rounded float64 result for every (Y, U, V))
 *     VP8HIP_RGB_BT601_FULL                0  256  359   -88  -183  454
 *     VP8HIP_RGB_BT709 (limited range)    16  298  459   -55  -136  541
 * The stream's color_space / clamping_type bits are not read: the matrix is the caller's choice (a VP8 stream with color_space 0
 * is BT.601, limited range).
 * dtype: VP8HIP_RGB_U8 the byte v; VP8HIP_RGB_F32 (float)((double)v * (double)scale[c] + (double)bias[c]) for colour c (R, G, B --
 * by colour, not by position; the product is exact in double, so fused or not gives the same float); VP8HIP_RGB_F16 that float
 * rounded to nearest-even.  scale and bias are read for the float types only.
 * layout, per frame, dense, frame i at dst + i * dst_stride BYTES: VP8HIP_RGB_PLANAR three planes [3][dst_h][dst_w] in the order
 * `order` gives (NCHW); VP8HIP_RGB_PACKED3 [dst_h][dst_w][3] (RGB24 / BGR24, channels last); VP8HIP_RGB_PACKED4 [dst_h][dst_w][4],
 * fourth byte 255, bytes only.  order: 0 = R, G, B; 1 = B, G, R.
 * Same rules as vp8hip_frames_scale_async: any list of frame buffers, repeats allowed, fbs reusable on return; enqueued on the
 * context's stream; each frame read in a form it has, none converted, no raster pool made for frames left as tiles; only bytes
 * inside [dst + i * dst_stride, + vp8hip_rgb_size) written.  -2 with nothing enqueued for n < 1, a frame buffer out of range, a size
 * outside 1..16383, a bad filter / matrix / layout / order / dtype, PACKED4 with a float type, dst_stride < size, a dst that is not
 * device memory of the context's device, frames that do not fit in dst's allocation, or a dst / dst_stride not aligned to the
 * element type (bytes: any alignment).  Whole-piece stores need dst_w % 4 == 0 and dst, dst_stride aligned to 4 bytes (planar and
 * packed bytes), 8 (halves) or 16 (floats, four-byte pixels) -- what a dense torch tensor gives; anything else is written element
 * by element, correctly but slowly.
 * At the display size the frame is read directly.  At any other size the scaler runs into a scratch of packed I420 that the context
 * owns and the conversion reads that: one chunk of at most 512 frames and at most 256 MB (fewer frames per chunk for large targets,
 * one at least), reused chunk after chunk in stream order, allocated on first need, reported by vp8hip_rgb_scratch_bytes, freed by
 * vp8hip_release_staging and vp8hip_destroy; it is the only device memory the call adds.
 * vp8hip_rgb_size: bytes of one frame; 0 for anything the call would refuse on p alone. */
enum { VP8HIP_RGB_BT601 = 0, VP8HIP_RGB_BT601_FULL = 1, VP8HIP_RGB_BT709 = 2 };
enum { VP8HIP_RGB_PLANAR = 0, VP8HIP_RGB_PACKED3 = 1, VP8HIP_RGB_PACKED4 = 2 };
enum { VP8HIP_RGB_U8 = 0, VP8HIP_RGB_F16 = 1, VP8HIP_RGB_F32 = 2 };
typedef struct vp8hip_rgb {
    int dst_w, dst_h, filter;      /* as vp8hip_frames_scale_async */
    int matrix, layout, order, dtype;
    float scale[3], bias[3];       /* by colour R, G, B; read for F16 / F32 only */
} vp8hip_rgb;
size_t vp8hip_rgb_size(const vp8hip_rgb *p);
int  vp8hip_frames_rgb_async(vp8hip_ctx *ctx, const int *fbs, int n, const vp8hip_rgb *p, void *dst, size_t dst_stride);
size_t vp8hip_rgb_scratch_bytes(const vp8hip_ctx *ctx);
/* What the decoder knows about a frame beside its pixels, for models on the device: motion vectors and macroblock modes as tensors.
 * Any n IR slots (slots: any order, repeats allowed; reusable when the call returns) -- slots, not frame buffers: that is where the
 * data lies (include/vp8_ir.h: the vp8ir_mbx records and mvs[nmb * 16]), whoever wrote them (vp8hip_ir_upload*, vp8hip_ir_copy,
 * vp8hip_entropy_decode; also on a vp8hip_configure_pooled context: the blocks are not read); the caller knows which slot it decoded
 * into which frame buffer.  Two tensors per frame, dense, frame i at dst + i * stride BYTES; either destination may be NULL, not both:
 *     mv    [2][gh][gw] of mv_dtype; channel 0 = x (the IR's col), channel 1 = y (row)
 *     info  [popcount(planes)][gh][gw] bytes, the planes in the order of their bits
 * The grid.  dst_w = dst_h = 0, the native grid: gw = 4 * mb_cols, gh = 4 * mb_rows, and cell (by, bx) is luma block
 * k = (by & 3) * 4 + (bx & 3) of macroblock (by >> 2, bx >> 2) -- the coded area, past the display size.  Otherwise gw = dst_w,
 * gh = dst_h, and output (y, x) takes the cell (by, bx) = (sy >> 2, sx >> 2) with, in integers (d_w x d_h: the display size),
 *     sx = ((2 * x + 1) * d_w) / (2 * dst_w)        sy = ((2 * y + 1) * d_h) / (2 * dst_h)
 * -- the source pixel under the output's centre: at the display size (x >> 2, y >> 2), so that the tensor lines up pixel for pixel
 * with vp8hip_frames_rgb_async's at the same size.
 * The cell's values, mb = by >> 2 times mb_cols + bx >> 2, m = the slot's record of mb, h = the slot's header as of the call:
 *     vector    mvs[mb * 16 + k] as stored: 1/8-pel units, not clamped to the frame, no sign-bias flip; (0, 0) in every cell of a key
 *               frame (h.frame_type 0: the slot's vector area is stale and is not read) and of a macroblock with m.ref_frame == 0
 *       VP8HIP_SIDE_I16  the stored int16 v
 *       VP8HIP_SIDE_F32  (float)((double)v * (double)scale[c]), c = 0 for x, 1 for y (the product is exact in double: one rounding)
 *       VP8HIP_SIDE_F16  that float rounded to nearest-even
 *     VP8HIP_SIDE_REF      m.ref_frame (VP8IR_INTRA_FRAME .. VP8IR_ALTREF_FRAME)
 *     VP8HIP_SIDE_MODE     m.y_mode, or 10 + m.b_modes[k] where m.y_mode == VP8IR_B_PRED
 *     VP8HIP_SIDE_SKIP     m.flags & VP8IR_MB_SKIP
 *     VP8HIP_SIDE_SEGMENT  m.segment_id as the record holds it
 *     VP8HIP_SIDE_QINDEX   h.base_qindex when !h.segmentation_enabled; else, with s = m.segment_id & 3, h.segment_quant[s] when
 *                          h.mb_segment_abs_delta and h.base_qindex + h.segment_quant[s] otherwise, clamped to 0..127
 *                          (mb_init_dequantizer, vp8/decoder/decodframe.c)
 *     VP8HIP_SIDE_CODED    vp8ir_block_kind(&m, k): 0 no residual, 1 a lone DC, 2 more
 * Enqueued on the context's stream like vp8hip_frames_rgb_async: a later vp8hip_ir_upload*, vp8hip_ir_copy or vp8hip_entropy_decode
 * that rewrites one of the slots runs behind it.  Only bytes inside [dst + i * stride, + size) are written.  No device memory is
 * added and no frame buffer is touched.  Returns -2 with nothing enqueued for n < 1; a slot out of range or one that holds no frame
 * of the context's size (never filled); one of dst_w, dst_h zero and the other not; a size outside 1..16383; a bad mv_dtype; unknown
 * plane bits; info_dst with planes == 0; both destinations NULL; a stride below the size; an mv_dst / mv_stride not aligned to the
 * element; a destination that is not device memory of the context's device or that cannot hold n frames.  Whole-piece stores need
 * gw % 4 == 0 and destination and stride aligned to 4 bytes (info), 8 (int16, halves) or 16 (floats); anything else is written
 * element by element, correctly but slowly.
 * vp8hip_side_mv_size / vp8hip_side_info_size: bytes of one frame's tensor (2 * gh * gw * element size; popcount(planes) * gh * gw);
 * 0 for what the call would refuse on p alone.  ctx is read for the native grid only and may be NULL for a sized one. */
enum { VP8HIP_SIDE_I16 = 0, VP8HIP_SIDE_F16 = 1, VP8HIP_SIDE_F32 = 2 };
#define VP8HIP_SIDE_REF 1      /* bit order = plane order */
#define VP8HIP_SIDE_MODE 2
#define VP8HIP_SIDE_SKIP 4
#define VP8HIP_SIDE_SEGMENT 8
#define VP8HIP_SIDE_QINDEX 16
#define VP8HIP_SIDE_CODED 32
typedef struct vp8hip_side {
    int dst_w, dst_h;          /* both 0: the native block grid, 4 * mb_cols x 4 * mb_rows; otherwise 1..16383 each */
    int mv_dtype;              /* VP8HIP_SIDE_I16 / F16 / F32 */
    unsigned planes;           /* VP8HIP_SIDE_* bits for the info tensor */
    float scale[2];            /* x, y; read for F16 / F32 only */
} vp8hip_side;
size_t vp8hip_side_mv_size(const vp8hip_ctx *ctx, const vp8hip_side *p);
size_t vp8hip_side_info_size(const vp8hip_ctx *ctx, const vp8hip_side *p);
int  vp8hip_frames_side_async(vp8hip_ctx *ctx, const int *slots, int n, const vp8hip_side *p, void *mv_dst, size_t mv_stride,
                              void *info_dst, size_t info_stride);
/* The third input of a model on the compressed domain, beside the picture and the motion vectors: the decoded RESIDUAL, as a tensor.
 * Any n IR slots (slots: any order, repeats allowed; reusable when the call returns), whoever wrote them (vp8hip_ir_upload*,
 * vp8hip_ir_copy, vp8hip_entropy_decode; on a vp8hip_configure_pooled context the blocks are read from the pool through the records'
 * sparse_first, exactly as vp8hip_decode reads them: valid until the caller resets the pool).  One dense tensor per frame, frame i at
 * dst + i * dst_stride BYTES.
 * The residual of a sample is the value the reference's decode_macroblock adds to the prediction before the clamp: the content of
 * the `short` it holds at that point.  Constants and order of operations: vp8/common/idctllm.c:28-204, vp8/common/idct_blk.c:20-86,
 * vp8/decoder/decodframe.c:252-304.  With m = the slot's record of the macroblock, h = the slot's header as of the call:
 *   - m.flags & VP8IR_MB_SKIP: 0 everywhere.
 *   - the factors y1dc, y1ac, y2dc, y2ac, uvdc, uvac: mb_init_dequantizer / vp8cx_init_de_quantizer for h and m.segment_id & 3
 *     (decodframe.c:50-109, quant_common.c; vp8o_mb_dequant in the oracle).
 *   - a macroblock with a Y2 block (m.y_mode neither B_PRED nor SPLITMV): with m.eobs[24] > 1 each Y2 coefficient times its factor
 *     (the first: y2dc, the others: y2ac) is truncated to int16, then vp8_short_inv_walsh4x4_c runs, its first pass stored to int16;
 *     otherwise a = (int16)(y2[0] * y2dc) and all sixteen DCs are (a + 3) >> 3 (vp8_short_inv_walsh4x4_1_c).  Luma block k then has
 *     that DC with factor 1 for its first coefficient, and its others with y1ac.
 *   - a block with eobs[k] > 1 (vp8_short_idct4x4llm_c): each coefficient times its factor (the first: the plane's dc factor, the
 *     others: its ac factor) truncated to int16; the vertical pass stored to int16; the horizontal pass ends with (x + 4) >> 3.
 *   - a block with eobs[k] <= 1: dc = (int16)(first coefficient * dc factor), every sample of the block (dc + 4) >> 3
 *     (vp8_dc_only_idct_add_c) -- also a Y2 macroblock's luma block with eobs[k] <= 1, which takes the WHT's DC; 0 for a block with
 *     neither a DC nor coefficients.
 *   - chroma the same with uvdc, uvac.  No Y2 for B_PRED / SPLITMV: luma with y1dc, y1ac.
 * dtype.  VP8HIP_RES_I16: the int16 as defined.  VP8HIP_RES_F32: (float)((double)v * (double)scale[c]) for plane c (Y, U, V; the
 * product is exact in double: one rounding).  VP8HIP_RES_F16: that float rounded to nearest-even.
 * layout.  VP8HIP_RES_I420: three planes back to back at their own sizes, Y gh x gw, then U and V ch x cw -- the raw data, for an
 * encoder or a transcoder.  VP8HIP_RES_PLANAR: [3][gh][gw], chroma replicated: U and V of output (y, x) are the chroma sample
 * (sy >> 1, sx >> 1) under the luma sample (sy, sx) it takes -- sample for sample vp8hip_frames_rgb_async's planar tensor at that size.
 * The grid.  dst_w = dst_h = 0, the native grid: the coded area, gw = 16 * mb_cols, gh = 16 * mb_rows, cw = gw / 2, ch = gh / 2,
 * every output its own sample.  Otherwise gw = dst_w, gh = dst_h, cw = (gw + 1) / 2, ch = (gh + 1) / 2 and, in integers (d_w x d_h:
 * the display size; dcw = (d_w + 1) / 2, dch = (d_h + 1) / 2):
 *     luma output (y, x) takes luma sample      (((2 * y + 1) * d_h) / (2 * gh),  ((2 * x + 1) * d_w) / (2 * gw))
 *     I420 chroma output (y, x) takes chroma sample (((2 * y + 1) * dch) / (2 * ch), ((2 * x + 1) * dcw) / (2 * cw))
 * -- at the display size both are the identity: a crop of the coded area.
 * Enqueued on the context's stream like vp8hip_frames_side_async: a later vp8hip_ir_upload*, vp8hip_ir_copy, vp8hip_entropy_decode or
 * vp8hip_pool_reset that rewrites what the call reads runs behind it.  Only bytes inside [dst + i * dst_stride, + size) are written.
 * No device memory is added and no frame buffer is touched.  A slot whose entropy status had bit 1 (the pool was empty) is read in
 * bounds and gives garbage, as for vp8hip_decode.  Returns -2 with nothing enqueued for n < 1; a slot out of range or one that holds
 * no frame of the context's size (never filled); one of dst_w, dst_h zero and the other not; a size outside 1..16383; a bad layout or
 * dtype; dst_stride below the size; a dst / dst_stride not aligned to the element; a destination that is not device memory of the
 * context's device or that cannot hold n frames.  Whole-piece stores need gw % 4 == 0 (the I420 layout's chroma planes: cw % 4 == 0)
 * and dst, dst_stride aligned to 8 bytes (int16, halves) or 16 (floats); anything else is written element by element, each once.
 * vp8hip_residual_size: bytes of one frame's tensor; 0 for what the call would refuse on p alone.  ctx is read for the native grid
 * only and may be NULL for a sized one. */
enum { VP8HIP_RES_I16 = 0, VP8HIP_RES_F16 = 1, VP8HIP_RES_F32 = 2 };
enum { VP8HIP_RES_I420 = 0, VP8HIP_RES_PLANAR = 1 };
typedef struct vp8hip_residual {
    int dst_w, dst_h;          /* both 0: the native grid, the coded area; otherwise 1..16383 each */
    int layout;                /* VP8HIP_RES_I420 / PLANAR */
    int dtype;                 /* VP8HIP_RES_I16 / F16 / F32 */
    float scale[3];            /* Y, U, V; read for F16 / F32 only */
} vp8hip_residual;
size_t vp8hip_residual_size(const vp8hip_ctx *ctx, const vp8hip_residual *p);
int  vp8hip_frames_residual_async(vp8hip_ctx *ctx, const int *slots, int n, const vp8hip_residual *p, void *dst, size_t dst_stride);
/* The TRANSFORM COEFFICIENTS of IR slots as tensors, for consumers on the device that want them as they are: frequency-domain models
 * (blocks as [frequency][block row][block column], often the first few of the scan only), forensics and quantiser estimation (the
 * levels as coded, per frequency), requantisers (levels plus factors).  A forward DCT of vp8hip_frames_residual_async's samples does
 * not give them: the reference's int16 truncations and >> 3 roundings do not invert.
 * Any n IR slots on vp8hip_frames_residual_async's terms: any order, repeats, any producer; on a vp8hip_configure_pooled context the
 * blocks are read from the pool; a starved slot is read in bounds and gives garbage; slot slots[i] goes to dst + i * dst_stride BYTES.
 * There is only the native grid, the coded area: coefficients are not resampled, a consumer crops by whole blocks.
 * Below R = mb_rows, C = mb_cols, m = the slot's record of the macroblock, h = the slot's header as of the call, the six factors those
 * of vp8hip_frames_residual_async (mb_init_dequantizer for h and m.segment_id & 3).  Position (v, u) of block k is the reference's
 * qcoeff[k * 16 + 4 * v + u] (the IR stores it at [u * 4 + v]).  "A Y2 macroblock": m.y_mode neither B_PRED nor SPLITMV.
 * stage VP8HIP_COEF_LEVELS, what the stream codes:
 *   - m.flags & VP8IR_MB_SKIP: 0 everywhere.  Not a Y2 macroblock: its Y2 plane is 0.
 *   - a block k < 24 with m.eobs[k] > 1: the sixteen values the slot's block holds; with m.eobs[k] == 1 its first coefficient alone,
 *     and only where vp8ir_block_kind(&m, k) is 1; every other block 0.
 *   - position (0, 0) of a luma block of a Y2 macroblock: 0, whatever the stream's bytes hold there (its DC is not coded there).
 *   - the Y2 block: with m.eobs[24] > 1 the sixteen values of m.y2, with m.eobs[24] == 1 its first alone, with 0 nothing.
 * stage VP8HIP_COEF_DEQUANT, the `short`s that enter the inverse transforms:
 *   - each LEVELS value times its factor (the first of a block: the dc factor, the others the ac factor; y1dc / y1ac, uvdc / uvac,
 *     y2dc / y2ac) truncated to int16 (vp8_dequantize_b_c);
 *   - but position (0, 0) of a luma block of a Y2 macroblock that is not skipped: that block's output of vp8_short_inv_walsh4x4_c --
 *     of vp8_short_inv_walsh4x4_1_c with m.eobs[24] <= 1 -- as vp8hip_frames_residual_async defines it, with factor 1.
 *   So vp8_short_idct4x4llm_c's arithmetic on a DEQUANT block gives vp8hip_frames_residual_async's block for EVERY block -- the full
 *   transform of a lone DC is (dc + 4) >> 3 everywhere, vp8_dc_only_idct_add_c's value -- and the inverse WHT of the DEQUANT Y2 block
 *   gives the luma DCs.
 * The tensor: the planes asked for (planes: VP8HIP_COEF_Y | _U | _V | _Y2) back to back in bit order, each dense.  With G = 4 for Y,
 * 2 for U and V, 1 for Y2 -- the blocks of a macroblock each way -- a plane is
 *   VP8HIP_COEF_CHANNELS  [nfreq][G * R][G * C]: channel j at (block row, block column) is position j = 4 * v + u of that block
 *                         (VP8HIP_COEF_RASTER), or position zigzag[j] (VP8HIP_COEF_ZIGZAG; the VP8 scan 0 1 4 8 5 2 3 6 9 12 13 10
 *                         7 11 14 15), for j < nfreq: the first nfreq of the order;
 *   VP8HIP_COEF_INPLACE   [4 * G * R][4 * G * C]: position (v, u) of block (by, bx) at (4 * by + v, 4 * bx + u) -- the residual's
 *                         geometry; needs nfreq == 16 and VP8HIP_COEF_RASTER.
 * dtype and scale: vp8hip_frames_residual_async's rule, scale[k] for plane k (Y, U, V, Y2): the int16 as defined, or
 * (float)((double)v * (double)scale[k]), or that float rounded to nearest-even as a half.
 * Whole-piece stores (8 bytes of int16 or halves, 16 of floats) go where a plane's row is a multiple of 4 elements and dst and
 * dst_stride are aligned to the piece; everywhere else -- CHANNELS: U and V with odd C, Y2 with C % 4 != 0 -- element by element, each
 * once.  Only bytes inside [dst + i * dst_stride, + size) are written.
 * Enqueued on the context's stream like vp8hip_frames_residual_async and ordered the same against later writers of the slots.  No
 * device memory is added and no frame buffer is touched.  Returns -2 with nothing enqueued for what vp8hip_frames_residual_async
 * refuses of slots and destination; a bad stage, layout, order or dtype; nfreq outside 1..16; INPLACE with nfreq != 16 or ZIGZAG; no
 * plane bit or an unknown one.
 * vp8hip_coef_size: bytes of one frame's tensor on ctx; 0 for the parameters the call refuses, and for a NULL (or not yet
 * configured) context: the grid is the context's.
 * vp8hip_dequant_factors: out[s] = y1dc, y1ac, y2dc, y2ac, uvdc, uvac of segment s for header h, what a consumer of LEVELS needs beside
 * them.  Host only: no context, no GPU.  Returns 0, or -2 for a null pointer. */
enum { VP8HIP_COEF_DEQUANT = 0, VP8HIP_COEF_LEVELS = 1 };          /* stage  */
enum { VP8HIP_COEF_CHANNELS = 0, VP8HIP_COEF_INPLACE = 1 };        /* layout */
enum { VP8HIP_COEF_RASTER = 0, VP8HIP_COEF_ZIGZAG = 1 };           /* order  */
#define VP8HIP_COEF_Y 1    /* bit order = plane order */
#define VP8HIP_COEF_U 2
#define VP8HIP_COEF_V 4
#define VP8HIP_COEF_Y2 8
typedef struct vp8hip_coef {
    int stage, layout, order;
    int nfreq;                 /* 1..16: channels kept, CHANNELS layout */
    unsigned planes;           /* VP8HIP_COEF_* bits, at least one */
    int dtype;                 /* VP8HIP_RES_I16 / F16 / F32 */
    float scale[4];            /* Y, U, V, Y2; float types only */
} vp8hip_coef;
size_t vp8hip_coef_size(const vp8hip_ctx *ctx, const vp8hip_coef *p);
int  vp8hip_frames_coef_async(vp8hip_ctx *ctx, const int *slots, int n, const vp8hip_coef *p, void *dst, size_t dst_stride);
int  vp8hip_dequant_factors(const vp8ir_frame_hdr *h, int16_t out[4][6]);
/* ACCUMULATED motion, for models that take a P frame's flow and residual relative to one anchor picture (CoViAR's accumulate=True):
 * every pixel traced back, hop by hop, through the frames it was predicted from to the key frame that started the group.
 * The TRACE of a frame is d_h * d_w dwords, row-major, over the display-size luma grid d_w x d_h of the context (no other size:
 * traces must chain exactly): pixel (y, x) holds x' in the low int16 and y' in the high int16, the position in the anchor picture
 * this pixel descends from -- packed pairs, so that a hop is one dword gather.  vp8hip_trace_size: 4 * d_w * d_h (0: no context, or
 * one not configured).
 * Traces live in a POOL in the caller's device memory: pool_frames traces, entry i at pool + i * pool_stride BYTES.  A job is the
 * vp8hip_job of vp8hip_decode with dst_fb and ref_fb[1..3] read as pool entries (-1: no trace; ref_fb[0] unused): a caller that
 * numbers pool entries like its frame buffers passes the very jobs it decoded with, and the trace follows vp8_refs' bookkeeping --
 * hidden frames, golden and altref updates -- with no code of its own.  Jobs of one call are independent, as for vp8hip_decode.
 * For a job with h = its slot's header as of the call, pixel (y, x), mb = (y >> 4) * mb_cols + (x >> 4), m = the slot's record of mb,
 * k = ((y >> 2) & 3) * 4 + ((x >> 2) & 3):
 *     h.frame_type == 0:  T(y, x) = (x, y): the frame is an anchor; its refs are not read.
 *     otherwise  r = m.ref_frame, v = mvs[mb * 16 + k] as stored (1/8 pel, no sign-bias flip); for an intra macroblock
 *                (m.ref_frame == 0) r = 1 and v = (0, 0): the pixel is held in place through the last frame.
 *                ref_fb[r] < 0 (or an m.ref_frame above 3):  T(y, x) = (x, y).
 *                otherwise, with arithmetic >>,
 *                    sx = clamp(x + ((v.col + 4) >> 3), 0, d_w - 1)      sy = clamp(y + ((v.row + 4) >> 3), 0, d_h - 1)
 *                    T(y, x) = pool[ref_fb[r]](sy, sx), the whole dword
 * -- the nearest whole pixel of the vector (ties up), the clamp standing for the border extension.  A concealed key frame says
 * inter in its header and is traced as one.  Trace values are data and never addresses: an uninitialised entry yields garbage and
 * nothing else, and by induction every value of a properly chained pool lies inside the picture.
 * Enqueued on the context's stream like vp8hip_frames_side_async; it reads the slots' records and vectors, not the blocks (also on a
 * vp8hip_configure_pooled context), and a later writer of those slots runs behind it.  Only bytes inside [pool + dst * pool_stride,
 * + size) are written.  No device memory is added and no frame buffer is touched.  Returns -2 with nothing enqueued for n < 1; a
 * slot out of range or never filled; pool_frames < 1; pool_stride below the size; pool or pool_stride not a multiple of 4; a pool
 * that is not device memory of the context's device or whose pool_frames entries do not fit its allocation; a dst_fb outside
 * 0 .. pool_frames - 1; a ref_fb[1..3] neither -1 nor in range; a dst_fb that is a ref of any job of the call or another job's
 * dst_fb.  Whole 16-byte stores need d_w % 4 == 0 and pool, pool_stride aligned to 16; otherwise dword by dword, each once.
 *
 * vp8hip_trace_flow_async: any n pool entries (idx: any order, repeats allowed) as tensors [2][gh][gw] of dtype, frame i at
 * dst + i * dst_stride BYTES.  dst_w = dst_h = 0: gw x gh = the display size; otherwise 1..16383 each, and output (y, x) takes trace
 * pixel (sy, sx) = (((2 * y + 1) * d_h) / (2 * gh), ((2 * x + 1) * d_w) / (2 * gw)), the centre map of vp8hip_frames_side_async.
 * Channel 0 is a = T.x(sy, sx) - sx, channel 1 is a = T.y(sy, sx) - sy: whole display pixels, signed as vp8hip_frames_side_async's
 * vectors are (after one hop with nothing clamped channel 0 is (v.col + 4) >> 3), so that at a given size the tensor lines up
 * element for element with vp8hip_frames_rgb_async's and vp8hip_frames_side_async's.  VP8HIP_SIDE_I16: a as an int16;
 * VP8HIP_SIDE_F32: (float)((double)a * (double)scale[c]); VP8HIP_SIDE_F16: that float rounded to nearest-even.  Same stream, same
 * promises.  Returns -2 with nothing enqueued for n < 1; what the trace call refuses of a pool; an idx outside the pool; one of dst_w,
 * dst_h zero and the other not; a size outside 1..16383; a bad dtype; dst_stride below the size; dst / dst_stride not aligned to the
 * element; a destination that is not device memory of the context's device or that cannot hold n frames.  Whole-piece stores need
 * gw % 4 == 0 and dst, dst_stride aligned to 8 bytes (int16, halves) or 16 (floats); otherwise element by element, each once.
 * vp8hip_trace_flow_size: bytes of one frame's tensor, 0 for what the call would refuse on p alone; ctx is read for the display size
 * only and may be NULL for a sized grid. */
typedef struct vp8hip_trace_flow {
    int dst_w, dst_h;          /* both 0: the display size; otherwise 1..16383 each */
    int dtype;                 /* VP8HIP_SIDE_I16 / F16 / F32 */
    float scale[2];            /* x, y; read for F16 / F32 only */
} vp8hip_trace_flow;
size_t vp8hip_trace_size(const vp8hip_ctx *ctx);
int  vp8hip_frames_trace_async(vp8hip_ctx *ctx, const vp8hip_job *jobs, int n, void *pool, size_t pool_stride, int pool_frames);
size_t vp8hip_trace_flow_size(const vp8hip_ctx *ctx, const vp8hip_trace_flow *p);
int  vp8hip_trace_flow_async(vp8hip_ctx *ctx, const int *idx, int n, const vp8hip_trace_flow *p, const void *pool, size_t pool_stride,
                             int pool_frames, void *dst, size_t dst_stride);
/* The ACCUMULATED RESIDUAL, the other half of accumulation: a frame minus its anchor picture gathered at the frame's trace -- the
 * difference to the group's key frame, not vp8hip_frames_residual_async's residual of one frame against its own prediction.
 * Any n jobs (any order, repeats allowed; reusable when the call returns), each naming the frame buffer that holds the frame, the pool
 * entry that holds its trace (vp8hip_frames_trace_async) and the frame buffer that holds the anchor picture, which the caller keeps
 * for the group (vp8hip_frame_copy after a key frame: vp8_refs hands the key frame's buffer on once golden and altref have moved).
 * One dense tensor [3][gh][gw] of dtype per job, frame i at dst + i * dst_stride BYTES.  dst_w = dst_h = 0: gw x gh = the display
 * size; otherwise 1..16383 each.  For output (y, x), with d_w x d_h the display size, in integers:
 *     sy = ((2 * y + 1) * d_h) / (2 * gh)      sx = ((2 * x + 1) * d_w) / (2 * gw)     (vp8hip_trace_flow_async's centre map; the
 *                                                                                       identity at the display size)
 *     t  = pool[trace](sy, sx), the whole dword
 *     ax = clamp((int16)(t & 0xffff), 0, d_w - 1)      ay = clamp((int16)(t >> 16), 0, d_h - 1)
 *     C(F, py, px) = the bytes R, G, B vp8hip_frames_rgb_async's convert gives with `matrix` for Y = F.y[py][px], U = F.u[py >> 1][px >> 1],
 *                    V likewise: element (py, px) of that call's U8 planar tensor of frame buffer F at the display size
 *     a[c] = C(fb, sy, sx)[c] - C(anchor_fb, ay, ax)[c]                                -255 .. 255
 * Plane p holds the colour `order` puts at position p (0 = R, G, B; 1 = B, G, R).  VP8HIP_RES_I16: a as an int16; VP8HIP_RES_F32:
 * (float)((double)a * (double)scale[c]), c by colour, not by position; VP8HIP_RES_F16: that float rounded to nearest-even.  At the
 * display size this is rgb_u8(fb) - rgb_u8(anchor_fb)[:, ay, ax], and at any size the tensor lines up element for element with
 * vp8hip_trace_flow_async's and vp8hip_frames_rgb_async's planar one.
 * THE CLAMP is what it looks like: here, unlike in the trace and flow calls, a trace value becomes an address.  It is applied to every
 * value before any address is formed, so a pool entry that nobody wrote yields garbage values and never a read outside the anchor's
 * picture.  A properly chained pool never needs it.
 * Same rules as its neighbours: enqueued on the context's stream -- a later launch that writes one of the frame buffers runs behind
 * it, traces written by an earlier vp8hip_frames_trace_async are seen --; each frame buffer read in a form it has (raster where it
 * exists, else tiles), the frame and the anchor independently of each other, none converted; no device memory added, no raster pool
 * made for frames left as tiles, no frame buffer and no pool entry written; only bytes inside [dst + i * dst_stride, + size) written.
 * Returns -2 with nothing enqueued for n < 1; an fb or anchor_fb out of range; what vp8hip_trace_flow_async refuses of a pool; a trace
 * outside 0 .. pool_frames - 1; one of dst_w, dst_h zero and the other not; a size outside 1..16383; a bad matrix, order or dtype;
 * dst_stride below the size; dst / dst_stride not aligned to the element; a destination that is not device memory of the context's
 * device or that cannot hold n frames.  Whole-piece stores need gw % 4 == 0 and dst, dst_stride aligned to 8 bytes (int16, halves) or
 * 16 (floats); anything else is written element by element, each once.
 * vp8hip_trace_residual_size: 3 * gh * gw * element size; 0 for what the call would refuse on p alone; ctx is read for the display
 * size only and may be NULL for a sized grid. */
typedef struct vp8hip_anchor_job {     /* one output frame */
    int32_t fb;                /* frame buffer that holds the frame */
    int32_t trace;             /* pool entry that holds its trace (vp8hip_frames_trace_async) */
    int32_t anchor_fb;         /* frame buffer that holds the anchor picture, kept by the caller for the group */
} vp8hip_anchor_job;
typedef struct vp8hip_trace_residual {
    int dst_w, dst_h;          /* both 0: the display size; otherwise 1..16383 each */
    int matrix, order;         /* VP8HIP_RGB_BT601 / _BT601_FULL / _BT709; 0 = R, G, B  1 = B, G, R: vp8hip_frames_rgb_async's */
    int dtype;                 /* VP8HIP_RES_I16 / F16 / F32 */
    float scale[3];            /* by colour R, G, B; read for F16 / F32 only */
} vp8hip_trace_residual;
size_t vp8hip_trace_residual_size(const vp8hip_ctx *ctx, const vp8hip_trace_residual *p);
int  vp8hip_trace_residual_async(vp8hip_ctx *ctx, const vp8hip_anchor_job *jobs, int n, const vp8hip_trace_residual *p,
                                 const void *pool, size_t pool_stride, int pool_frames, void *dst, size_t dst_stride);
/* The GATHER ALONG THE TRACE: a tensor of the caller's carried from the anchor picture to a later frame -- what inference with codec
 * motion does with the result a heavy network gave for the key frame (feature maps of any stride, logits, a label map).  Any n jobs
 * (any order, repeats allowed; reusable when the call returns), each naming the pool entry that holds a frame's trace
 * (vp8hip_frames_trace_async) and one of src_frames SOURCE TENSORS, tensor k at src + k * src_stride BYTES; output i at
 * dst + i * dst_stride BYTES.  Both are the caller's device memory and dense, `channels` elements of `elem` bytes per cell:
 * VP8HIP_GATHER_PLANAR [C][h][w], VP8HIP_GATHER_CHANNELS_LAST [h][w][C]; the output has the source's layout and element size.  No frame
 * buffer and no IR slot is read.  With d_w x d_h the display size, sw x sh = src_w x src_h the source grid and gw x gh the output grid
 * (dst_w = dst_h = 0: the display size; otherwise 1..16383 each), for output (y, x), in integers:
 *     sy = ((2 * y + 1) * d_h) / (2 * gh)      sx = ((2 * x + 1) * d_w) / (2 * gw)     (vp8hip_trace_flow_async's centre map; the
 *                                                                                       identity at the display size)
 *     t  = pool[trace](sy, sx), the whole dword
 *     ax = clamp((int16)(t & 0xffff), 0, d_w - 1)      ay = clamp((int16)(t >> 16), 0, d_h - 1)
 *     NEAREST:   cx = ((2 * ax + 1) * sw) / (2 * d_w)      cy = ((2 * ay + 1) * sh) / (2 * d_h)      the cell under the anchor pixel's centre
 *                out[c](y, x) = src[c](cy, cx), the element's bits, for every c
 *     BILINEAR:  px = clamp(((2 * ax + 1) * sw * 128) / d_w - 128, 0, (sw - 1) * 256)      (64-bit) the pixel's centre in 1/256 cells,
 *                x0 = px >> 8, wx = px & 255, x1 = min(x0 + 1, sw - 1); py, y0, wy, y1 likewise       counted from the cells' centres
 *                R  = (a (256 - wx)(256 - wy) + b wx (256 - wy) + c' (256 - wx) wy + d wx wy) / 65536   in real numbers,
 *                     a = src(y0, x0), b = src(y0, x1), c' = src(y1, x0), d = src(y1, x1)
 * With sw = d_w / s for a stride s that divides d_w, cx == ax / s.  cx is monotone in ax; for sw <= d_w it takes every cell 0 .. sw - 1,
 * and for sw > d_w the d_w pixels name d_w different cells (they cannot name more).  With sw == d_w every wx is 0, so BILINEAR equals
 * NEAREST bit for bit (likewise sh, wy).  With all four weights on one corner the output is that corner's value exactly, for finite
 * inputs.
 * NEAREST moves bits of any meaning.  BILINEAR reads elements of 2 bytes as IEEE halves and of 4 as floats, refuses 1, works in single
 * precision and delivers a value within a derived bound of R, M = max(|a|, |b|, |c'|, |d|):
 *     floats:  |out - R| <= 8 * 2^-24 * M                         both natural orders (two lerps then one; four weighted products summed) make at
 *                                                                 most six roundings of relative error 2^-24 on magnitudes <= M; a third is left over
 *     halves:  |out - R| <= 8 * 2^-24 * M + 2^-11 * |R| + 2^-25   widened exactly, float arithmetic (the first term), one rounding to the
 *                                                                 nearest-even half (the second), half the smallest subnormal half (the third)
 * Non-finite inputs give unspecified values and nothing else.
 * THE CLAMP: as in vp8hip_trace_residual_async a trace value becomes an address.  Every value is clamped before any address is formed,
 * and cx < sw, cy < sh, x1 < sw, y1 < sh follow from the formulas: a pool entry nobody wrote yields garbage values and never a read
 * outside the job's source tensor.
 * Same rules as its neighbours: enqueued on the context's stream, so traces written by an earlier vp8hip_frames_trace_async are seen;
 * no device memory added; no pool entry, source tensor or frame buffer written; only bytes inside [dst + i * dst_stride, + size)
 * written.  Returns -2 with nothing enqueued for n < 1; what vp8hip_trace_flow_async refuses of a pool; a trace outside
 * 0 .. pool_frames - 1 or a src outside 0 .. src_frames - 1; one of dst_w, dst_h zero and the other not; a size outside 1..16383;
 * src_w or src_h outside 1..16383; channels outside 1..4096; an elem other than 1, 2, 4; a bad layout or filter; BILINEAR with
 * elem == 1; src_stride or dst_stride below its tensor's size; src, dst or their strides not aligned to the element; src or dst that
 * is not device memory of the context's device or whose frames do not fit the allocation; [src, + src_frames * src_stride)
 * overlapping [dst, + n * dst_stride).  Whole-piece stores: PLANAR needs gw % 4 == 0 and dst, dst_stride aligned to 4 * elem;
 * CHANNELS_LAST needs channels * elem, dst, dst_stride, src and src_stride to be multiples of 16; anything else is written element by
 * element, each once.
 * The source is checked by the code that checks destinations: an error text that begins "vp8hip_trace_gather_async (src)" and speaks of
 * "the destination" means src and src_stride.
 * vp8hip_trace_gather_size: channels * gh * gw * elem, the bytes of one output; 0 for what the call would refuse on p alone; ctx is
 * read for the display size only and may be NULL for a sized grid. */
typedef struct vp8hip_gather_job {     /* one output */
    int32_t trace;             /* pool entry that holds the frame's trace (vp8hip_frames_trace_async) */
    int32_t src;               /* index of the source tensor */
} vp8hip_gather_job;
enum { VP8HIP_GATHER_NEAREST = 0, VP8HIP_GATHER_BILINEAR = 1 };
enum { VP8HIP_GATHER_PLANAR = 0, VP8HIP_GATHER_CHANNELS_LAST = 1 };
typedef struct vp8hip_trace_gather {
    int dst_w, dst_h;          /* both 0: the display size; otherwise 1..16383 each */
    int src_w, src_h;          /* the source tensors' grid, 1..16383 each: a feature map of any stride, or the picture's size */
    int channels;              /* 1..4096 */
    int elem;                  /* bytes of an element: 1, 2 or 4.  NEAREST moves bits; BILINEAR reads 2 as IEEE halves, 4 as floats, refuses 1 */
    int layout, filter;        /* VP8HIP_GATHER_PLANAR / _CHANNELS_LAST; VP8HIP_GATHER_NEAREST / _BILINEAR */
} vp8hip_trace_gather;
size_t vp8hip_trace_gather_size(const vp8hip_ctx *ctx, const vp8hip_trace_gather *p);
int  vp8hip_trace_gather_async(vp8hip_ctx *ctx, const vp8hip_gather_job *jobs, int n, const vp8hip_trace_gather *p,
                               const void *pool, size_t pool_stride, int pool_frames,
                               const void *src, size_t src_stride, int src_frames, void *dst, size_t dst_stride);
/* TRACE WEAR: where what vp8hip_trace_gather_async carried is still true.  The trace always gives an answer, also where the answer is
 * a fiction -- an intra macroblock of an inter frame is "held in place", a vector that leaves the picture is clamped, a block with a
 * coded residual was corrected after the copy, every hop rounds its vector to whole pixels -- and the methods that propagate a key
 * frame's result decide per region when to stop trusting it.  The WEAR of a frame counts those events along the very chain its trace
 * follows: d_h * d_w dwords, row-major, over the display-size luma grid -- a trace's shape and size (vp8hip_trace_size) -- pixel (y, x)
 * holding four saturating byte counters, byte b in bits 8b .. 8b + 7, of the hops on the way to the anchor in which
 *     byte 0  HOPS    anything happened: every hop
 *     byte 1  INTRA   the pixel's macroblock was intra (held in place: no correspondence)
 *     byte 2  EDGE    the clamp moved the position (predicted from border replication)
 *     byte 3  CODED   the pixel's luma block may have had a non-zero residual
 * Wear entries live in a POOL in the caller's device memory with a trace pool's rules (pool_frames entries, pool_stride BYTES apart,
 * dword-aligned), numbered like the caller's trace pool and frame buffers.  A job is the vp8hip_job, read exactly as
 * vp8hip_frames_trace_async reads it.  For a job with h = its slot's header as of the call and pixel (y, x), with mb, m, k, r, v as in
 * the trace's definition (an intra macroblock: r = 1, v = (0, 0)):
 *     h.frame_type == 0:  W(y, x) = 0; the records are not read.
 *     ref_fb[r] < 0 (or an m.ref_frame above 3):  W(y, x) = 0: the trace is the identity there, the frame counts as an anchor.
 *     otherwise, with arithmetic >>,
 *         ux = x + ((v.col + 4) >> 3)          uy = y + ((v.row + 4) >> 3)
 *         sx = clamp(ux, 0, d_w - 1)           sy = clamp(uy, 0, d_h - 1)
 *         P  = pool[ref_fb[r]](sy, sx), the whole dword
 *         inc = (1,  m.ref_frame == 0,  sx != ux || sy != uy,
 *                !(m.flags & VP8IR_MB_SKIP) && (vp8ir_block_kind(&m, k) != 0 || vp8ir_block_kind(&m, 24) != 0))
 *         W(y, x).byte[b] = min(P.byte[b] + inc[b], 255)
 * CODED is conservative on purpose: in a macroblock with a Y2 block a luma block with nothing of its own still gets a DC through the
 * WHT, and vp8ir_block_kind(m, 24) is 0 for B_PRED / SPLITMV, so an increment of 0 means the pixel's luma residual is exactly zero.
 * Not counted: the sub-pixel part of a vector (the interpolation filters), the chroma residual, the loop filter.
 * Wear values are data and never addresses: an entry nobody wrote yields garbage counters and nothing else; the positions that become
 * addresses come from the slot's vectors, after the clamp.
 * vp8hip_frames_wear_async has vp8hip_frames_trace_async's promises and refusals: enqueued on the context's stream; it reads the slots'
 * records and vectors, not the blocks (also on a vp8hip_configure_pooled context), and a later writer of those slots runs behind it;
 * only bytes inside [pool + dst * pool_stride, + size) are written; no device memory is added and no frame buffer is touched.  Returns
 * -2 with nothing enqueued for n < 1; a slot out of range or never filled; pool_frames < 1; pool_stride below the size; pool or
 * pool_stride not a multiple of 4; a pool that is not device memory of the context's device or whose pool_frames entries do not fit its
 * allocation; a dst_fb outside 0 .. pool_frames - 1; a ref_fb[1..3] neither -1 nor in range; a dst_fb that is a ref of any job of the
 * call or another job's dst_fb.  Whole 16-byte stores need d_w % 4 == 0 and pool, pool_stride aligned to 16; otherwise dword by dword,
 * each once.
 *
 * vp8hip_trace_wear_async: any n pool entries (idx: any order, repeats allowed) as tensors [popcount(planes)][gh][gw] of dtype, the
 * planes in bit order, frame i at dst + i * dst_stride BYTES.  dst_w = dst_h = 0: gw x gh = the display size; otherwise 1..16383 each,
 * and output (y, x) takes wear pixel (sy, sx) by vp8hip_trace_flow_async's centre map, so that at a given size the tensor lines up
 * element for element with vp8hip_trace_flow_async's, vp8hip_trace_residual_async's, vp8hip_trace_gather_async's and
 * vp8hip_frames_rgb_async's.  With v the byte of counter c: VP8HIP_WEAR_U8: v; VP8HIP_WEAR_F32: (float)((double)v * (double)scale[c]);
 * VP8HIP_WEAR_F16: that float rounded to nearest-even.  Same stream, same promises; no pool entry written.  Returns -2 with nothing
 * enqueued for what vp8hip_trace_flow_async refuses (n < 1; a pool; an idx outside it; the sizes; a bad dtype; the destination), and
 * for planes == 0 or bits other than VP8HIP_WEAR_*.  Whole-piece stores need gw % 4 == 0 and dst, dst_stride aligned to 4 bytes
 * (bytes), 8 (halves) or 16 (floats); anything else is written element by element, each once.
 * vp8hip_trace_wear_size: popcount(planes) * gh * gw * element size; 0 for what the call would refuse on p alone; ctx is read for the
 * display size only and may be NULL for a sized grid. */
enum { VP8HIP_WEAR_U8 = 0, VP8HIP_WEAR_F16 = 1, VP8HIP_WEAR_F32 = 2 };
#define VP8HIP_WEAR_HOPS  1      /* bit order = plane order */
#define VP8HIP_WEAR_INTRA 2
#define VP8HIP_WEAR_EDGE  4
#define VP8HIP_WEAR_CODED 8
typedef struct vp8hip_trace_wear {
    int dst_w, dst_h;          /* both 0: the display size; otherwise 1..16383 each */
    int dtype;                 /* VP8HIP_WEAR_U8 / F16 / F32 */
    unsigned planes;           /* VP8HIP_WEAR_* bits, at least one */
    float scale[4];            /* by counter (HOPS, INTRA, EDGE, CODED), not by position; read for F16 / F32 only */
} vp8hip_trace_wear;
int  vp8hip_frames_wear_async(vp8hip_ctx *ctx, const vp8hip_job *jobs, int n, void *pool, size_t pool_stride, int pool_frames);
size_t vp8hip_trace_wear_size(const vp8hip_ctx *ctx, const vp8hip_trace_wear *p);
int  vp8hip_trace_wear_async(vp8hip_ctx *ctx, const int *idx, int n, const vp8hip_trace_wear *p, const void *pool, size_t pool_stride,
                             int pool_frames, void *dst, size_t dst_stride);
/* A TRACE INVERTED: first descendant and descendant count per anchor pixel.  The trace and everything made from it face one way: for a
 * pixel of a later frame, what is true about it in the anchor picture.  The inverse answers the opposite question -- for a pixel of the
 * anchor picture, did it survive into the frame, where is it now, and how many pixels of the frame claim it -- which is what pushing
 * boxes, keypoints and track seeds forward, telling a stretched region from a covered one, and warping a later frame's tensors onto the
 * anchor's grid need.  With d_w x d_h the context's display size and T a trace pool entry:
 *   - For a frame pixel p = (y, x), a(p) = trace_clamp(T(y, x)) = (ay, ax):
 *         ax = clamp((int16)(t & 0xffff), 0, d_w - 1)      ay = clamp((int16)(t >> 16), 0, d_h - 1)
 *     the one clamp the readers of a trace share.
 *   - D(a) is the set of frame pixels p with a(p) = a.
 * Two outputs are defined per job.  Each has a trace entry's shape and size: vp8hip_trace_size, d_h * d_w dwords, row-major over the
 * anchor's grid.
 *   - FIRST(ay, ax):
 *       - It is the member of D(a) that comes first in raster order, packed as a trace packs a position (x in the low int16, y in the
 *         high one).
 *       - It is 0xffffffff where D(a) is empty.
 *       - Positions are non-negative and below 16384.  So unsigned order of the packed dword IS raster order, and 0xffffffff is above
 *         every position.  FIRST is the unsigned minimum over D(a) of y << 16 | x.
 *       - A FIRST entry is therefore a trace in the other direction.  vp8hip_trace_flow_async and vp8hip_trace_gather_async read a
 *         FIRST pool unchanged.  The gather then forward-warps a frame-t tensor onto the anchor grid.
 *       - Where D(a) is empty they read (-1, -1).  Their existing definitions handle that value: it is data, clamped to (0, 0) before
 *         it is an address.  COUNT is the mask for it.
 *   - COUNT(ay, ax) = |D(a)|, an exact uint32.  It is at most d_w * d_h, which is below 2^28.
 *   - The sum of COUNT over the entry is d_w * d_h.
 * Both are pure functions of the trace entry.  They are unsigned min and integer add, so the result does not depend on the order in
 * which lanes arrive.  Two runs give the same bits.
 * vp8hip_trace_invert_async: `first` and `count` are pools in the caller's device memory with a trace pool's rules (out_frames entries
 * each, first_stride / count_stride BYTES apart, dword-aligned, strides at least the entry size, inside one allocation of the context's
 * device).  Either may be NULL, not both.  Job i reads pool[trace] and writes entry dst of each pool given; repeats of `trace` are
 * allowed.  Enqueued on the context's stream: traces written by an earlier vp8hip_frames_trace_async are seen.  The call adds no device
 * memory and reads no slot and no frame buffer; only bytes inside the dst entries are written.  THE CLAMP guards writes here: every
 * trace value is clamped before an address is formed from it, so a trace entry nobody wrote scatters garbage inside the job's
 * destination entries and nowhere else.  Returns -2 with nothing enqueued for n < 1; what vp8hip_trace_flow_async refuses of a pool,
 * for each of the three pools; a trace outside 0 .. pool_frames - 1 or a dst outside 0 .. out_frames - 1; two jobs with one dst; both
 * outputs NULL; any two of the three byte ranges [pool, + pool_frames * pool_stride), [first, + out_frames * first_stride),
 * [count, + out_frames * count_stride) overlapping (vp8hip_trace_gather_async's rule for src / dst).
 *
 * vp8hip_trace_cover_async: any n entries of a COUNT pool (idx: any order, repeats allowed) as tensors [popcount(planes)][gh][gw] of
 * dtype (VP8HIP_WEAR_U8 / F16 / F32), the planes in bit order, frame i at dst + i * dst_stride BYTES, under vp8hip_trace_flow_async's
 * centre map: vp8hip_trace_wear_async's shape over a COUNT pool.  With c the count under the output's centre: VP8HIP_COVER_COUNT has
 * v = min(c, 255), VP8HIP_COVER_SEEN has v = (c != 0).  U8 gives v; F32 (float)((double)v * (double)scale[plane]), by plane (COUNT,
 * SEEN), not by position; F16 that float rounded to nearest-even.  v saturates at 255 for every dtype, as wear's counters do: these
 * are compared with small thresholds, and the exact dwords are in the caller's pool already.  Refusals, alignment rules and
 * whole-piece stores are those of vp8hip_trace_wear_async, with VP8HIP_COVER_* for its planes.
 * vp8hip_trace_cover_size: popcount(planes) * gh * gw * element size; 0 for what the call would refuse on p alone; ctx is read for the
 * display size only and may be NULL for a sized grid. */
typedef struct vp8hip_invert_job {     /* one inverted trace */
    int32_t trace;             /* pool entry that holds the frame's trace (vp8hip_frames_trace_async) */
    int32_t dst;               /* entry of the FIRST pool and of the COUNT pool written */
} vp8hip_invert_job;
int  vp8hip_trace_invert_async(vp8hip_ctx *ctx, const vp8hip_invert_job *jobs, int n,
                               const void *pool, size_t pool_stride, int pool_frames,      /* traces, read */
                               void *first, size_t first_stride, void *count, size_t count_stride, int out_frames);
#define VP8HIP_COVER_COUNT 1     /* bit order = plane order */
#define VP8HIP_COVER_SEEN  2
typedef struct vp8hip_trace_cover {
    int dst_w, dst_h;          /* both 0: the display size; otherwise 1..16383 each */
    int dtype;                 /* VP8HIP_WEAR_U8 / F16 / F32 */
    unsigned planes;           /* VP8HIP_COVER_* bits, at least one */
    float scale[2];            /* by plane (COUNT, SEEN), not by position; read for F16 / F32 only */
} vp8hip_trace_cover;
size_t vp8hip_trace_cover_size(const vp8hip_ctx *ctx, const vp8hip_trace_cover *p);
int  vp8hip_trace_cover_async(vp8hip_ctx *ctx, const int *idx, int n, const vp8hip_trace_cover *p, const void *count, size_t count_stride,
                              int count_frames, void *dst, size_t dst_stride);
/* FRAME SUMMARIES: byte histograms of pictures, slots, wear and cover.  Everything above hands a device consumer a per-pixel tensor;
 * the decisions a pipeline makes around those tensors are per frame -- is this a scene cut, is the picture black or frozen, how far is
 * it from the anchor, has the trace worn out, what share of the frame is intra.  A 256-bin histogram is the exact reduction of byte
 * data: from H[k] the caller derives count, sum, mean, variance, any percentile and any threshold share without loss, and from the
 * histogram of |a - b| SAD, SSE, PSNR and "how many samples moved by more than t".  Each of the four calls is defined as the histogram
 * of a U8 tensor an existing call gives; that tensor is never made.
 * Every output has one shape: [popcount(planes)][256] of uint32, the planes in the order of their bits, output i at
 * dst + i * dst_stride BYTES in the caller's device memory; vp8hip_hist_size(popcount) = popcount * 1024, 0 for a popcount outside
 * 1..32.  Every plane's 256 counts sum to the number of elements counted; a count is at most 16383^2 < 2^28.  The result is integer
 * counting: the same bits in every run, whatever order lanes and workgroups arrive in.
 *
 * vp8hip_frames_hist_async: let S(F) be the packed I420 image vp8hip_frames_scale_async writes for frame buffer F at the display size:
 * luma d_w x d_h, chroma ((d_w + 1) / 2) x ((d_h + 1) / 2).  Job i with ref_fb < 0: H[p][k] = the number of samples of plane p of
 * S(fb) equal to k.  With ref_fb >= 0: the number of sample positions where |S(fb) - S(ref_fb)| equals k.  planes: VP8HIP_HIST_Y, _U,
 * _V.  Each frame buffer is read in a form it has -- raster where it exists, else tiles; the two of a pair independently; one never
 * written reads as zeros --, nothing is converted or allocated, and no raster pool is made for frames left as tiles.  Jobs come in
 * any order, with repeats; fb == ref_fb is legal and puts everything into bin 0.
 *
 * vp8hip_slots_hist_async: H[p][k] = the number of cells of the NATIVE grid (4 * mb_cols x 4 * mb_rows) whose value in plane p of
 * vp8hip_frames_side_async's info tensor equals k: the planes VP8HIP_SIDE_REF, _MODE, _SKIP, _SEGMENT, _QINDEX and _CODED exactly as
 * defined there, with the slot's header as of the call.  VP8HIP_HIST_MVMAG (this call only; vp8hip_frames_side_async keeps refusing
 * bit 64) is a seventh plane, behind the six: with (vx, vy) the cell's vector as that call's I16 tensor holds it -- (0, 0) on key
 * frames and intra macroblocks --, px = (vx + 4) >> 3 and py = (vy + 4) >> 3 (arithmetic shifts: the trace's rounding to whole
 * pixels), the value is min(max(|px|, |py|), 255).  The call reads records and vectors, not blocks: also on a
 * vp8hip_configure_pooled context.
 *
 * vp8hip_trace_wear_hist_async / vp8hip_trace_cover_hist_async: H[p][k] = the number of pixels of entry idx[i] (all d_w * d_h) whose
 * value in plane p of vp8hip_trace_wear_async's / vp8hip_trace_cover_async's U8 tensor at the display size equals k.  planes:
 * VP8HIP_WEAR_* / VP8HIP_COVER_*; COUNT saturates at 255 and SEEN fills bins 0 and 1 only.  Pool values are data and never addresses.
 *
 * All four are their neighbours: enqueued on the context's stream -- a later writer of a frame buffer, slot or pool entry runs behind
 * the call, and an earlier vp8hip_decode, vp8hip_frames_wear_async or vp8hip_trace_invert_async is seen --; no device memory is added;
 * no frame buffer, slot or pool entry is written; only bytes inside [dst + i * dst_stride, + size) are written.  They return -2 with
 * nothing enqueued for n < 1; an fb, slot or idx out of range, or a slot never filled; a ref_fb neither -1 nor in range; planes == 0
 * or bits the call does not know; what vp8hip_trace_flow_async refuses of a pool; dst_stride below the size; dst or dst_stride not a
 * multiple of 4; a destination that is not device memory of the context's device or that cannot hold n outputs; and, for the two pool
 * calls, [dst, + n * dst_stride) overlapping the pool. */
#define VP8HIP_HIST_Y 1          /* bit order = plane order */
#define VP8HIP_HIST_U 2
#define VP8HIP_HIST_V 4
#define VP8HIP_HIST_MVMAG 64     /* beside the VP8HIP_SIDE_* bits, for vp8hip_slots_hist_async only */
typedef struct vp8hip_hist_job {       /* one output */
    int32_t fb;                /* the frame buffer counted */
    int32_t ref_fb;            /* -1: none; otherwise the frame buffer it is compared with */
} vp8hip_hist_job;
size_t vp8hip_hist_size(int planes_popcount);
int  vp8hip_frames_hist_async(vp8hip_ctx *ctx, const vp8hip_hist_job *jobs, int n, unsigned planes, void *dst, size_t dst_stride);
int  vp8hip_slots_hist_async(vp8hip_ctx *ctx, const int *slots, int n, unsigned planes, void *dst, size_t dst_stride);
int  vp8hip_trace_wear_hist_async(vp8hip_ctx *ctx, const int *idx, int n, unsigned planes, const void *pool, size_t pool_stride,
                                  int pool_frames, void *dst, size_t dst_stride);
int  vp8hip_trace_cover_hist_async(vp8hip_ctx *ctx, const int *idx, int n, unsigned planes, const void *count, size_t count_stride,
                                   int count_frames, void *dst, size_t dst_stride);
/* STRUCTURAL SIMILARITY of picture pairs.  SSIM cannot be had from any histogram: it needs the joint second moments of two pictures
 * over local windows.  vp8hip_frames_ssim_async computes what the reference reports beside PSNR for a picture pair (vp8_calc_ssim /
 * vp8_calc_ssimg, vp8/encoder/ssim.c: vp8_ssim2 per plane, 8x8 windows on the 4-pixel grid "to penalize blocking artifacts") in
 * the reference's integer definition, for any n jobs of vp8hip_hist_job (fb, ref_fb), in any order, with repeats.  ref_fb must be a
 * frame buffer (-1 is refused); fb == ref_fb is legal.  The planes are those of vp8hip_frames_hist_async -- S(F), the display-size
 * I420 image: luma d_w x d_h, chroma ((d_w + 1) / 2) x ((d_h + 1) / 2) --, chosen with VP8HIP_HIST_Y | _U | _V, in bit order.
 *
 * WINDOWS.  A plane of pw x ph has a window with its top left sample at row 4 * wy, column 4 * wx for every 4 * wy < ph - 8 and
 * 4 * wx < pw - 8 -- vp8_ssim2's loop, strict < included: the last aligned window is left out as the reference leaves it out --,
 * that is nwx = pw > 8 ? (pw - 5) / 4 : 0 columns and likewise nwy rows of windows (vp8hip_ssim_windows: host only, no context and
 * no GPU; -2, and 0 x 0, for a size outside 1..16383).  Every window lies inside the display-size plane and nothing outside it is
 * read.  A plane with pw <= 8 or ph <= 8 has no windows (the reference returns 0 / 0 there).
 *
 * VALUE.  With the five sums over a window's 64 samples (s from fb, r from ref_fb) in signed 64-bit integers, c1 = 26634 and
 * c2 = 239708 (similarity() with count 64):
 *     n = (2 * Ss * Sr + c1) * (2 * 64 * Ssr - 2 * Ss * Sr + c2)
 *     d = (Ss * Ss + Sr * Sr + c1) * (64 * Sss - Ss * Ss + 64 * Srr - Sr * Sr + c2)
 *     v = (double)n / (double)d
 * the two conversions rounded to nearest and the division IEEE-correct.  Always d > 0 and |v| <= 1 (Cauchy-Schwarz on both factors).
 *
 * OUTPUTS, either of which may be NULL, not both:
 *   scores  [popcount(planes)][2] of int64, job i at scores + i * scores_stride BYTES (both multiples of 8;
 *           vp8hip_ssim_scores_size(popcount) = 16 * popcount, 0 for a popcount outside 1..3): [p][0] = the sum over the plane's
 *           windows of llrint(v * 2^32) (round half to even; the product is exact), [p][1] = the number of windows, nwx * nwy.  The
 *           sum is in integers: the same bits in every run, whatever order lanes and workgroups arrive in.  The mean is
 *           [p][0] / 2^32 / [p][1]; it differs from vp8_ssim2's result by at most 2^-33 + N * 2^-52 (the rounding to Q32, and the
 *           reference's own summation of N doubles).  |total| < 2^57.  fb == ref_fb gives exactly count << 32.
 *   map     the planes asked for, back to back, plane p a dense [nwy_p][nwx_p] of map_dtype, job i at map + i * map_stride BYTES
 *           (both aligned to the element): VP8HIP_SSIM_F32 is (float)v, VP8HIP_SSIM_F16 that float rounded to nearest-even.
 *           vp8hip_ssim_map_size(ctx, p): the bytes of one job's map, 0 for what the call refuses on p alone (and for a NULL or
 *           unconfigured ctx).  Every element is written once, element by element, the lanes of a wave on neighbouring windows of
 *           a row.  map_dtype is 0 (no map: only where map is NULL), VP8HIP_SSIM_F16 or VP8HIP_SSIM_F32.
 *
 * The call is its neighbours: enqueued on the context's stream -- a later writer of a frame buffer runs behind it, an earlier
 * vp8hip_decode is seen --; each frame buffer is read in a form it has (raster where it exists, else tiles; the two of a pair
 * independently; one never written reads as zeros), nothing is converted, no raster pool is made and no device memory is added; no
 * frame buffer is written; only bytes inside [scores + i * scores_stride, + size) and [map + i * map_stride, + size) are written.
 * It returns -2 with nothing enqueued for n < 1; an fb or ref_fb out of range (ref_fb < 0 included); planes == 0 or bits other than
 * VP8HIP_HIST_Y | _U | _V; both destinations NULL; a map asked for when no plane asked for has a window; a map_dtype other than
 * the above, or 0 with a map; a stride below the size; a destination or stride not aligned (scores: 8, map: the element); a
 * destination that is not device memory of the context's device or that cannot hold n outputs; scores and map that overlap.
 *
 * vp8hip_ssim_share(ctx, n, planes): how many workgroups share each job of a call of n jobs over `planes` on this context -- the
 * call's own arithmetic.  1: a workgroup owns a job and stores its scores; more: the scores are first set to {0, count} and the
 * workgroups add their sums to them.  0 for what the call refuses of n and planes.  The results do not depend on it. */
#define VP8HIP_SSIM_F16 1
#define VP8HIP_SSIM_F32 2
typedef struct vp8hip_ssim {
    unsigned planes;           /* VP8HIP_HIST_Y | _U | _V, at least one */
    int map_dtype;             /* 0 (no map), VP8HIP_SSIM_F16, VP8HIP_SSIM_F32 */
} vp8hip_ssim;
int  vp8hip_ssim_windows(int w, int h, int *nwx, int *nwy);
size_t vp8hip_ssim_scores_size(int planes_popcount);
size_t vp8hip_ssim_map_size(const vp8hip_ctx *ctx, const vp8hip_ssim *p);
int  vp8hip_ssim_share(const vp8hip_ctx *ctx, int n, unsigned planes);
int  vp8hip_frames_ssim_async(vp8hip_ctx *ctx, const vp8hip_hist_job *jobs, int n, const vp8hip_ssim *p, void *scores, size_t scores_stride,
                              void *map, size_t map_stride);
/* BLOCK MOTION SEARCH between pictures.  What the stream codes of motion (vp8hip_frames_side_async, the traces) exists only for
 * inter macroblocks, only between a frame and its references, and is a rate-distortion choice.  vp8hip_frames_motion_async computes,
 * per macroblock of ANY picture pair, the best whole-pixel displacement and what that match costs: the reference's exhaustive
 * search, vp8_full_search_sad_c (vp8/encoder/mcomp.c) over vp8_sad16x16_c, with vp8_variance16x16_c at the result, bit for bit.
 * Jobs are vp8hip_hist_job (fb, ref_fb), any n, in any order, with repeats: fb holds the blocks (the reference's `what`), ref_fb is
 * searched (`in_what`); ref_fb < 0 is refused; fb == ref_fb is legal.  Luma only, 16x16 only, whole pixels only.
 *
 * PICTURES.  A = 16 * mb_cols and B = 16 * mb_rows are the coded luma size.  S(F)(y, x), 0 <= y < B, 0 <= x < A, is the decoded luma of
 * frame buffer F over the coded area, read in a form F has -- raster where it exists, else tiles; the two of a pair independently;
 * a buffer never written reads as zeros.  E(F)(y, x) = S(F)(clamp(y, 0, B - 1), clamp(x, 0, A - 1)) for any y, x: the edge
 * replication the reference's border extension gives, by coordinate clamps -- the raster form's borders are never read, and both
 * forms give the same bits.
 *
 * Per macroblock (my, mx), with the distance d = p->distance in 1..64:
 *   BOUNDS  cmin = -(16 mx + 16), cmax = 16 (mb_cols - 1 - mx) + 16, rmin = -(16 my + 16), rmax = 16 (mb_rows - 1 - my) + 16: the
 *           reference's mv_col_min .. mv_row_max with VP8BORDERINPIXELS - 16 = 16 (vp8/encoder/encodeframe.c).
 *   CENTRE  (cy, cx) in whole pixels: (0, 0) where `centre` is NULL; otherwise read from the caller's tensor in device memory,
 *           [2][mb_rows][mb_cols] of int16, channel 0 = x, channel 1 = y, job i's at centre + i * centre_stride BYTES (both multiples
 *           of 2), and clamped, cx to [cmin, cmax], cy to [rmin, rmax].  The value is data, never an address.  A caller seeds the
 *           search with vp8hip_frames_side_async's vectors (>> 3) or with a coarser search of its own.  A centre tensor is refused on
 *           a context of more than 255 macroblocks a side, where a clamped centre << 3 would leave int16.
 *   CANDIDATES, in this order: the centre; then r from max(cy - d, rmin) up to but NOT including min(cy + d, rmax) and inside it c
 *           from max(cx - d, cmin) up to but NOT including min(cx + d, cmax).  The exclusive upper ends are the reference's loop
 *           (r < row_max, c < col_max): the row cy + d and the column cx + d are never searched, nor are the row rmax and the
 *           column cmax unless the centre lies on them.  That omission is the reference's and is kept.
 *   VALUE   of the candidate (r, c): sum over y, x in 0..15 of |S(fb)(16 my + y, 16 mx + x) - E(ref_fb)(16 my + r + y, 16 mx + c + x)|
 *           plus, with a cost table, ((cost[0][r - cy + d] + cost[1][c - cx + d]) * sad_per_bit + 128) >> 8: mvsad_err_cost with the
 *           cost centre at the search centre.  p->cost is a HOST pointer to int32 [2][2 d + 1] (row costs, then column costs; the last
 *           entry of each, index 2 d, is never reached), entries 0..65535, copied at the call; sad_per_bit is 0..255.  cost == NULL
 *           or sad_per_bit == 0: no cost term (and cost is not read).
 *   BEST    the first candidate in that order whose value is strictly below all before it (the reference's `thissad < bestsad`): on a
 *           flat block the centre, among equal values of the loop the first in raster order.  The reduction is by the key (value,
 *           position in the order): the same bits in every run, whatever order lanes and waves arrive in.
 *
 * OUTPUTS, either of which may be NULL, not both; both dense per job on the macroblock grid:
 *   mv      [2][mb_rows][mb_cols] of int16, job i at mv + i * mv_stride BYTES (both multiples of 2): channel 0 = c_best << 3,
 *           channel 1 = r_best << 3 -- the units and the channel order of vp8hip_frames_side_async's I16 tensor, so that the two can
 *           be compared or mixed element for element.  vp8hip_motion_mv_size(ctx) = 4 * mb_rows * mb_cols (0 for a NULL or
 *           unconfigured ctx); it is the centre tensor's size too.
 *   stats   [popcount(p->planes)][mb_rows][mb_cols] of uint32, job i at stats + i * stats_stride BYTES (both multiples of 4), the
 *           planes in the order of their bits:
 *             VP8HIP_MOTION_SAD     the best value, cost term included;
 *             VP8HIP_MOTION_SAD0    the plain sum of absolute differences at the vector (0, 0), whatever the centre;
 *             VP8HIP_MOTION_SSE     the sum of squared differences at the best candidate;
 *             VP8HIP_MOTION_VAR     sse - (uint32)(((int64)sum * sum) >> 8) at the best candidate, sum the signed sum of differences:
 *                                   vp8_variance16x16_c, written in 64 bits.  The reference's `int` product overflows for
 *                                   |sum| > 46340 (a block within about 75 levels of 0 against one within about 75 of 255); there the
 *                                   two differ, and this is the one without the overflow;
 *             VP8HIP_MOTION_SRCVAR  the same formula for the block of fb against the constant 128: the spatial activity the
 *                                   reference's encoder takes from vp8_variance16x16(src, VP8_VAR_OFFS, 0); |sum| <= 32768.
 *           vp8hip_motion_stats_size(ctx, p) = 4 * popcount * mb_rows * mb_cols; 0 for what the call refuses on p alone (planes == 0
 *           included) and for a NULL or unconfigured ctx.  p->planes is not read where stats is NULL, except for unknown bits.
 *
 * The call is its neighbours: enqueued on the context's stream -- a later writer of a frame buffer runs behind it, an earlier
 * vp8hip_decode is seen --; nothing is converted, no raster pool is made and no device memory is added; no frame buffer is written;
 * only bytes inside [mv + i * mv_stride, + size) and [stats + i * stats_stride, + size) are written.  It returns -2 with nothing
 * enqueued for n < 1; an fb or ref_fb out of range (ref_fb < 0 included); a distance outside 1..64; plane bits other than the
 * five; stats with planes == 0; both outputs NULL; a cost entry outside 0..65535 (where the table is read) or a sad_per_bit outside
 * 0..255; a stride below the size; a pointer or stride not aligned (mv: 2, stats: 4, centre: 2); an output or a centre tensor that
 * is not device memory of the context's device or that cannot hold n jobs; outputs that overlap each other or the centre tensor; a
 * centre tensor on more than 255 macroblocks a side. */
#define VP8HIP_MOTION_SAD    1   /* bit order = plane order */
#define VP8HIP_MOTION_SAD0   2
#define VP8HIP_MOTION_SSE    4
#define VP8HIP_MOTION_VAR    8
#define VP8HIP_MOTION_SRCVAR 16
typedef struct vp8hip_motion {
    int distance;              /* 1..64 */
    int sad_per_bit;           /* 0..255; 0: no cost term */
    unsigned planes;           /* VP8HIP_MOTION_* bits of stats; may be 0 where stats is NULL */
    const int32_t *cost;       /* host memory, int32 [2][2 * distance + 1], or NULL: no cost term */
} vp8hip_motion;
size_t vp8hip_motion_mv_size(const vp8hip_ctx *ctx);
size_t vp8hip_motion_stats_size(const vp8hip_ctx *ctx, const vp8hip_motion *p);
int  vp8hip_frames_motion_async(vp8hip_ctx *ctx, const vp8hip_hist_job *jobs, int n, const vp8hip_motion *p, const void *centre,
                                size_t centre_stride, void *mv, size_t mv_stride, void *stats, size_t stats_stride);
/* SUB-PIXEL REFINEMENT of block motion between pictures.  vp8hip_frames_motion_async's vectors are whole pixels; everything else
 * that carries motion here (vp8hip_frames_side_async, the traces, the flow tensors) has quarter-pel precision in 1/8-pel units.
 * vp8hip_frames_subpel_async is the step the reference always makes behind its whole-pixel search: vp8_find_best_sub_pixel_step
 * (vp8/encoder/mcomp.c; at precision 2 vp8_find_best_half_pixel_step, the same code cut short) over
 * vp8_sub_pixel_variance16x16_c, bit for bit.  Jobs are vp8hip_hist_job (fb, ref_fb) exactly as for vp8hip_frames_motion_async, and
 * so are the pictures S(F), E(F), A, B and how a frame buffer is read; ref_fb < 0 is refused, fb == ref_fb is legal.  Luma only,
 * 16x16 only.
 *
 * Per macroblock (my, mx), with the motion call's BOUNDS cmin, cmax, rmin, rmax:
 *   START   (sy, sx) in whole pixels: (0, 0) where `start` is NULL; otherwise read from the caller's tensor in device memory,
 *           [2][mb_rows][mb_cols] of int16, channel 0 = x, channel 1 = y, in 1/8 PEL -- vp8hip_frames_motion_async's mv output as it
 *           stands --, job i's at start + i * start_stride BYTES (both multiples of 2); each component is shifted >> 3
 *           arithmetically, then clamped, sx to [cmin, cmax], sy to [rmin, rmax].  The value is data, never an address.  A start
 *           tensor is refused on a context of more than 255 macroblocks a side, where 8 * a clamped start would leave int16.
 *   PREDICTION at a vector v = (vy, vx) in 1/8 pel, both components even: with the base (by, bx) = (vy >> 3, vx >> 3)
 *           (arithmetic shifts) and the offsets (oy, ox) = (vy & 7, vx & 7), and Y = 16 my + by, X = 16 mx + bx,
 *             H(y, x) = (E(ref_fb)(Y + y, X + x) * (128 - 16 ox) + E(ref_fb)(Y + y, X + x + 1) * 16 ox + 64) >> 7, y in 0..16, x in 0..15,
 *             P(y, x) = (H(y, x) * (128 - 16 oy) + H(y + 1, x) * 16 oy + 64) >> 7,                            y, x in 0..15:
 *           vp8_sub_pixel_variance16x16_c's predictor with vp8_bilinear_filters[o] = {128 - 16 o, 16 o}, the horizontal pass
 *           rounded before the vertical one.  Both passes are always made, also at offset 0 (the filter {128, 0}: the input comes
 *           through).  Over the eleven candidates below the pixels touched lie in rows and columns s - 1 .. s + 16 of the block's
 *           position at the start: 18 x 18.
 *   DIST(v) = sse - (uint32)(((int64)sum * sum) >> 8), sse and sum the sums over y, x in 0..15 of the squared and of the signed
 *           difference between S(fb)(16 my + y, 16 mx + x) and P(y, x): vp8_variance16x16_c, written in 64 bits as
 *           VP8HIP_MOTION_VAR is.  The reference's `int` product overflows for |sum| > 46340; there the two differ, and this is the
 *           one without the overflow.
 *   COST(v) = ((cost[0][iy] + cost[1][ix]) * error_per_bit + 128) >> 8 with a cost table -- the reference's mv_err_cost --, else 0;
 *           iy = clamp((vy - ry) >> 1, -R, R) + R and ix = clamp((vx - rx) >> 1, -R, R) + R (arithmetic shifts), (ry, rx) the
 *           REFERENCE VECTOR the cost is counted from: (0, 0) where `ref` is NULL, otherwise read from a tensor of start's shape
 *           and units (any int16; job i's at ref + i * ref_stride BYTES), and read only where there is a cost term.  The clamp to
 *           +-R is this library's: the reference would read outside its table there.  p->cost is a HOST pointer to int32
 *           [2][2 R + 1] (row costs, then column costs), entries 0..65535, with R = p->cost_range in 1..1023 (the reference's mv_max);
 *           p->error_per_bit is 0..16383, so the product stays inside int32.  cost == NULL or error_per_bit == 0: no cost term, and
 *           neither the table nor cost_range nor `ref` is read.  The table is copied at the call: the caller may change it on
 *           return, and two calls queued back to back with different tables each see their own.
 *   ORDER   the reference's.  With v0 = (8 sy, 8 sx) the best starts as v0, valued DIST + COST like every candidate.  Stage 1, with
 *           h = 4 around c = v0: left c + (0, -h), right c + (0, +h), up c + (-h, 0), down c + (+h, 0) are valued in that order, and
 *           each replaces the best only when STRICTLY below it; then one diagonal c + (up < down ? -h : +h, left < right ? -h : +h)
 *           -- the reference's whichdir = (left < right ? 0 : 1) + (up < down ? 0 : 2): 0 up-left, 1 up-right, 2 down-left, 3
 *           down-right; the comparisons are between the four values themselves, ties go right and down -- is valued and replaces
 *           the best when strictly below it.  Stage 2 is the same with h = 2 around c = the best of stage 1.  p->precision == 2
 *           stops after stage 1, p->precision == 4 runs both: six or eleven evaluations.  No bounds are applied to the sub-pixel
 *           candidates (the reference's step applies none): a vector can end 6/8 pel past a UMV bound, and E is defined there.
 *
 * OUTPUTS, either of which may be NULL, not both; both dense per job on the macroblock grid:
 *   mv      [2][mb_rows][mb_cols] of int16, job i at mv + i * mv_stride BYTES (both multiples of 2): channel 0 = x, channel 1 = y of
 *           the best vector in 1/8 pel: comparable element for element with vp8hip_frames_side_async's I16 tensor and with
 *           vp8hip_frames_motion_async's.  vp8hip_subpel_mv_size(ctx) = 4 * mb_rows * mb_cols (0 for a NULL or unconfigured ctx); it
 *           is the size of the start and of the ref tensor too.
 *   stats   [popcount(p->planes)][mb_rows][mb_cols] of uint32, job i at stats + i * stats_stride BYTES (both multiples of 4), the
 *           planes in the order of their bits:
 *             VP8HIP_SUBPEL_VAL     the best value, cost term included: what the reference's function returns;
 *             VP8HIP_SUBPEL_VAR     DIST at the best vector (the reference's *distortion);
 *             VP8HIP_SUBPEL_SSE     sse at the best vector (*sse1);
 *             VP8HIP_SUBPEL_VAR0    DIST at v0: what the refinement started from.
 *           vp8hip_subpel_stats_size(ctx, p) = 4 * popcount * mb_rows * mb_cols; 0 for a precision, an error_per_bit or planes the
 *           call refuses (planes == 0 included) and for a NULL or unconfigured ctx.  p->planes is not read where stats is NULL,
 *           except for unknown bits.
 *
 * The call is its neighbours: enqueued on the context's stream -- a later writer of a frame buffer runs behind it, an earlier
 * vp8hip_decode is seen --; nothing is converted, no raster pool is made; no frame buffer is written; only bytes inside
 * [mv + i * mv_stride, + size) and [stats + i * stats_stride, + size) are written.  Without a cost term it adds no device memory.
 * With one, the table (up to 8188 bytes as uint16) goes to a copy the context owns: 8 KB of device memory, made by the first call
 * that has a table and freed with the context -- the call's one allocation; the table travels there in the arguments of small
 * launches ahead of the kernel, so nothing is synchronised.  It returns -2 with nothing enqueued for n < 1; an fb or ref_fb out of
 * range (ref_fb < 0 included); a precision other than 2 and 4; an error_per_bit outside 0..16383; plane bits other than the four;
 * stats with planes == 0; both outputs NULL; where the table is read, a cost_range outside 1..1023 or an entry outside 0..65535; a
 * stride below the size; a pointer or stride not aligned (mv, start, ref: 2, stats: 4); an output, a start or a ref tensor that is
 * not device memory of the context's device or that cannot hold n jobs; outputs that overlap each other or the start or the ref
 * tensor (start and ref may be the same memory); a start tensor on more than 255 macroblocks a side. */
#define VP8HIP_SUBPEL_VAL    1   /* bit order = plane order */
#define VP8HIP_SUBPEL_VAR    2
#define VP8HIP_SUBPEL_SSE    4
#define VP8HIP_SUBPEL_VAR0   8
typedef struct vp8hip_subpel {
    int precision;             /* 2: the half-pixel stage alone; 4: both stages */
    int error_per_bit;         /* 0..16383; 0: no cost term */
    int cost_range;            /* R, 1..1023: a row of the table has 2 R + 1 entries; read with the table */
    unsigned planes;           /* VP8HIP_SUBPEL_* bits of stats; may be 0 where stats is NULL */
    const int32_t *cost;       /* host memory, int32 [2][2 * cost_range + 1], or NULL: no cost term */
} vp8hip_subpel;
size_t vp8hip_subpel_mv_size(const vp8hip_ctx *ctx);
size_t vp8hip_subpel_stats_size(const vp8hip_ctx *ctx, const vp8hip_subpel *p);
int  vp8hip_frames_subpel_async(vp8hip_ctx *ctx, const vp8hip_hist_job *jobs, int n, const vp8hip_subpel *p, const void *start,
                                size_t start_stride, const void *ref, size_t ref_stride, void *mv, size_t mv_stride, void *stats,
                                size_t stats_stride);
/* MOTION-COMPENSATED TEMPORAL FILTER of pictures (ARNR).  The two calls above end in vectors and error figures; this one makes a
 * picture of them: the reference's alt-ref noise-reduction filter (vp8/encoder/temporal_filter.c), which blends the motion-
 * compensated predictions from neighbouring pictures into a centre picture pixel by pixel, trusting a prediction less the further
 * it lies from the centre's pixel -- vp8_temporal_filter_predictors_mb_c followed by vp8_temporal_filter_apply_c per source, then
 * the normalisation by cpi->fixed_divide, bit for bit, for all three planes.
 *
 * PAIRS AND JOBS.  `pairs` is the very list a caller gave vp8hip_frames_motion_async / _subpel_async: pair k = (fb, ref_fb), ref_fb
 * the SOURCE picture.  Job i filters the centre picture jobs[i].fb over the pairs first .. first + count - 1, in that order; count is
 * 1..15 (the reference's arnr_max_frames); every pair in that range must have fb == jobs[i].fb.  Jobs may share or repeat pairs.  The
 * centre itself takes part only where the caller lists the pair (fb, fb) (the reference always has it, at vector (0, 0) and error 0).
 *
 * INPUTS, in device memory, either of which may be NULL:
 *   mv      pair k's tensor [2][mb_rows][mb_cols] of int16 at mv + k * mv_stride BYTES (both multiples of 2), channel 0 = x,
 *           channel 1 = y, in 1/8 pel: vp8hip_frames_subpel_async's or vp8hip_frames_motion_async's output as it stands (the
 *           reference's d->bmi.mv).  Any int16 value is legal, odd ones included; a vector is data, never an address.  NULL: (0, 0)
 *           everywhere, the reference with ALT_REF_MC_ENABLED off.
 *   err     pair k's plane [mb_rows][mb_cols] of uint32 at err + k * err_stride BYTES (both multiples of 4):
 *           vp8hip_frames_subpel_async's VAL plane (the reference's bestsme).  The WEIGHT of source k for a macroblock is
 *           W = err < thresh_low ? 2 : err < thresh_high ? 1 : 0, compared UNSIGNED; the reference compares an int, and the two agree
 *           for every err below 2^31.  NULL: W = 2 everywhere.  A source whose W is 0 for a macroblock adds nothing to it.
 *
 * PICTURES.  S(F), E(F), A, B and how a frame buffer is read are as for vp8hip_frames_motion_async, now for all three planes: chroma's
 * coded area is A/2 x B/2, extended by coordinate clamps as luma is.
 *
 * Per macroblock (my, mx), source k with vector (vy, vx) and weight W != 0:
 *   LUMA    the prediction P is 16x16, its base (Y, X) = (16 my + (vy >> 3), 16 mx + (vx >> 3)) and its offsets (oy, ox) =
 *           (vy & 7, vx & 7), arithmetic shifts.  Where both offsets are 0, P(y, x) = E(ref_fb)(Y + y, X + x) (vp8_copy_mem16x16).
 *           Otherwise, with VP8HIP_TFILTER_SIXTAP, vp8_sixtap_predict16x16_c: with f = vp8_sub_pel_filters[ox],
 *             H(y, x) = clamp255((sum over t in 0..5 of E(ref_fb)(Y + y, X + x + t - 2) * f[t] + 64) >> 7), y in -2..18, x in 0..15,
 *           and with f = vp8_sub_pel_filters[oy], P(y, x) = clamp255((sum over t of H(y + t - 2, x) * f[t] + 64) >> 7): the
 *           horizontal pass rounded and clamped to bytes before the vertical one, both always made, the pass-through filter
 *           {0, 0, 128, 0, 0, 0} of offset 0 included.  With VP8HIP_TFILTER_BILINEAR, vp8_bilinear_predict16x16_c: 17 rows
 *           H(y, x) = (E(Y + y, X + x) * (128 - 16 ox) + E(Y + y, X + x + 1) * 16 ox + 64) >> 7, then
 *           P(y, x) = (H(y, x) * (128 - 16 oy) + H(y + 1, x) * 16 oy + 64) >> 7 (vp8_bilinear_filters).
 *   CHROMA  the vector is (cy, cx) = (vy >> 1, vx >> 1), arithmetic: the temporal filter's own rule -- no full-pixel rounding, and
 *           all eight phases occur.  U and V are 8x8, base (8 my + (cy >> 3), 8 mx + (cx >> 3)), offsets (cy & 7, cx & 7), through
 *           the 8x8 functions in the same way (13 or 9 rows); whether they are copied is decided by the chroma offsets.
 *   BLEND   per pixel of the three blocks, with s the centre's pixel from S(fb) and q the prediction's:
 *             m = ((s - q)^2 * 3 + r) >> strength,  r = 1 << (strength - 1), and r = 0 at strength 0
 *             m = (16 - min(m, 16)) * W;   count += m;   accumulator += m * q.
 *           At strength 0 the reference shifts by -1, which C leaves undefined; r = 0 there (m = 3 (s - q)^2) is THIS LIBRARY'S
 *           definition.
 * After the last source: pixel = ((accumulator + (count >> 1)) * (count ? 0x80000 / count : 0)) >> 19 in uint32, its low byte --
 * cpi->fixed_divide.  A count of 0 gives 0.  count <= 15 * 32 = 480, inside the reference's table of 512.
 *
 * OUTPUTS, in the caller's device memory; either may be NULL, not both:
 *   dst     job i's picture at dst + i * dst_stride BYTES, packed I420 at the DISPLAY size, vp8hip_i420_size(w, h) bytes:
 *           vp8hip_frames_scale_async's layout at the native size.  The coded area's right and bottom surplus is computed but not
 *           stored.
 *   cnt     the same geometry in uint16 at cnt + i * cnt_stride BYTES (both multiples of 2): the per-pixel count, the support the
 *           pixel got; 32 per fully trusted source.  vp8hip_tfilter_count_size(ctx) = 2 * vp8hip_i420_size(w, h) (0 for a NULL or
 *           unconfigured ctx).
 *
 * The call is its neighbours: enqueued on the context's stream -- a later writer of a frame buffer runs behind it, an earlier
 * vp8hip_decode is seen --; nothing is converted, no raster pool is made and no device memory is added; no frame buffer is written;
 * only bytes inside [dst + i * dst_stride, + size) and [cnt + i * cnt_stride, + size) are written; no atomics: the same bits in every
 * run.  It returns -2 with nothing enqueued for n < 1 or npairs < 1; an fb or ref_fb out of range; a count outside 1..15; a range
 * outside `pairs`; a pair whose fb is not the job's; a strength outside 0..6; an unknown filter; thresh_high < thresh_low; both
 * outputs NULL; a stride below the size; a pointer or stride not aligned (mv: 2, err: 4, cnt: 2); an output, mv or err that is not
 * device memory of the context's device or that cannot hold its n (outputs) or npairs (inputs) items; outputs that overlap each
 * other or an input.  Writing the result back into a frame buffer, and RGB of the result, are not part of it. */
#define VP8HIP_TFILTER_SIXTAP   0
#define VP8HIP_TFILTER_BILINEAR 1
typedef struct vp8hip_tfilter {
    int strength;              /* 0..6: the reference's arnr_strength */
    int filter;                /* VP8HIP_TFILTER_SIXTAP / _BILINEAR */
    unsigned thresh_low;       /* the reference's THRESH_LOW, 10000 */
    unsigned thresh_high;      /* the reference's THRESH_HIGH, 20000; >= thresh_low */
} vp8hip_tfilter;
typedef struct vp8hip_tfilter_job { int32_t fb, first, count; } vp8hip_tfilter_job;
size_t vp8hip_tfilter_count_size(const vp8hip_ctx *ctx);
int  vp8hip_frames_tfilter_async(vp8hip_ctx *ctx, const vp8hip_tfilter_job *jobs, int n, const vp8hip_hist_job *pairs, int npairs,
                                 const vp8hip_tfilter *p, const void *mv, size_t mv_stride, const void *err, size_t err_stride,
                                 void *dst, size_t dst_stride, void *cnt, size_t cnt_stride);
/* TRANSFORM AND QUANTISATION of the motion-compensated residual of picture pairs.  What the reference does with a 16x16 vector
 * inside its mode decision and its encode loop is always the same five steps -- predict, subtract, forward DCT and Walsh transform,
 * quantise, then dequantise, inverse-transform and add: vp8_encode_inter16x16 (vp8/encoder/encodemb.c) followed by
 * vp8_inverse_transform_mby and vp8_dequant_idct_add_uv_block.  vp8hip_frames_quant_async makes them per macroblock of any picture
 * pair, bit for bit, and hands out the levels, the end-of-block positions, the error figures and the reconstruction: from pictures
 * to what an entropy coder, a requantiser or a rate-distortion estimate reads, without leaving the device.  SPLITMV, intra modes (vp8hip_frames_intra_async below),
 * the trellis (optimize_b), tokens and rate in bits, per-macroblock quantisers and the loop filter are not part of it.
 *
 * JOBS are vp8hip_hist_job (fb, ref_fb) exactly as for vp8hip_frames_subpel_async: fb is the SOURCE picture, ref_fb the REFERENCE it is
 * predicted from; ref_fb < 0 is refused, fb == ref_fb is legal.  S(F), E(F), the coded area A x B and how a frame buffer in either
 * form is read are vp8hip_frames_tfilter_async's, for all three planes.
 *
 * VECTORS.  mv is a device pointer, or NULL for (0, 0) everywhere: job i's tensor [2][mb_rows][mb_cols] of int16 at
 * mv + i * mv_stride BYTES (both multiples of 2), channel 0 = x, channel 1 = y, in 1/8 pel -- vp8hip_frames_subpel_async's or
 * vp8hip_frames_motion_async's output as it stands: the reference's mbmi.mv.  Any int16 is legal and is data, never an address.  No
 * clamp to the UMV border is applied (the reference with need_to_clamp_mvs 0); E is defined everywhere.
 *
 * QUANTISER.  p->qindex, 0..127, applies to every job; where p->job_qindex is not NULL it is a HOST pointer to n bytes, copied at the
 * call, job i's qindex (each 0..127; p->qindex is then not read).  p->delta[5] = y1dc, y2dc, y2ac, uvdc, uvac, each -15..15, as a
 * frame header carries them, passed in explicitly: the rule of the reference's vp8_set_quantizer that y2dc is 4 - Q below Q 4 (and 0
 * from there) is the CALLER'S to apply.  The factors are vp8hip_quant_factors(qindex, delta) below.  p->quantizer:
 *   VP8HIP_QUANT_REGULAR  vp8_regular_quantize_b_c as the reference compiles it (EXACT_QUANT), over the improved_quant tables;
 *   VP8HIP_QUANT_FAST     vp8_fast_quantize_b_c as compiled (without EXACT_FASTQUANT), over quant_fast, with no zero bin.
 * The zero bin of the regular form is widened by three terms that keep the reference's names: p->zbin_over_quant,
 * p->zbin_mode_boost, p->act_zbin_adj, each -1048576..1048576 (so that nothing below overflows an int; the reference's own values
 * are 0..192, 0..12 and -1..4), combined as the reference's ZBIN_EXTRA macros combine them and truncated as its `(short)` does:
 *   extra_Y = (short)((Y1 dequant ac * (zbin_over_quant + zbin_mode_boost + act_zbin_adj)) >> 7), extra_UV the same with UV dequant ac,
 *   extra_Y2 = (short)((Y2 dequant ac * (zbin_over_quant / 2 + zbin_mode_boost + act_zbin_adj)) >> 7), the division C's (towards 0).
 * They are not read by the fast form.  p->filter is VP8HIP_TFILTER_SIXTAP or VP8HIP_TFILTER_BILINEAR, with
 * vp8hip_frames_tfilter_async's meaning.
 *
 * Per macroblock (my, mx) with the vector (vy, vx), in the reference's order:
 *   1. PREDICTION, vp8_build_inter16x16_predictors_mb.  Luma is exactly vp8hip_frames_tfilter_async's LUMA paragraph: a copy, the
 *      six-tap or the bilinear filter by the offsets (vy & 7, vx & 7).  Chroma is NOT that call's rule but the decoder's: each
 *      component c of the luma vector becomes (c + (c < 0 ? -1 : 1)) / 2 with C's truncating division, no full-pixel mask; then base
 *      >> 3 and offset & 7 through the 8x8 functions as there, and whether chroma is copied is decided by ITS offsets.  The
 *      reference makes the += +-1 in a `short`, which wraps at 32767 and -32768; here it is made in int without the wrap: the two
 *      differ for those two values only (32767 gives 16384 here and -16384 there, -32768 gives -16384 here and 16383 there).
 *   2. RESIDUAL, vp8_subtract_mby_c and vp8_subtract_mbuv_c: source minus prediction, int16.
 *   3. TRANSFORM, transform_mb for a 16x16 mode: vp8_short_fdct4x4_c on the 24 blocks -- block 4 r + c of luma at rows 4 r, columns
 *      4 c of the macroblock, U 16 + 2 r + c, V 20 + 2 r + c likewise in their 8x8 --, with its four rounding constants and the
 *      + (d1 != 0) on row 1; then the sixteen luma blocks' coefficient 0 (build_dcblock) through vp8_short_walsh4x4_c, with its
 *      + (a1 != 0) and its += (x < 0) before (x + 3) >> 3, into block 24.  A luma block's own coefficient 0 stays what the DCT made
 *      it -- the reference does not clear it --, so the quantiser quantises it with the y1dc factors, and it counts in that block's
 *      eob: an entropy coder skips position 0 of the luma blocks of a macroblock that has a Y2 block, as every macroblock here has.
 *   4. QUANTISATION of the 25 blocks, sixteen steps in zigzag order (0 1 4 8 5 2 3 6 9 12 13 10 7 11 14 15), position 0 with the dc
 *      factors, the others with the ac factors of the block's table (Y1 for blocks 0..15, UV for 16..23, Y2 for 24), x = |z|:
 *        regular:  zbin = zbin + zrun_zbin_boost[run] + extra;  y = x >= zbin ? (((x + round) * quant >> 16) + x + round) >> quant_shift : 0;
 *                  run = y ? 0 : run + 1 (the number of steps since the last non-zero level, 0 at the start);
 *        fast:     y = ((x + round) * quant_fast) >> 16;
 *      qcoeff = z < 0 ? -y : y, dqcoeff = (int16)(qcoeff * dequant), eob = 1 + the last step whose y is not 0, else 0.
 *   5. RECONSTRUCTION on the prediction of step 1.  vp8_inverse_transform_mby: vp8_short_inv_walsh4x4_c of block 24's dqcoeff where
 *      eob[24] > 1, vp8_short_inv_walsh4x4_1_c ((dqcoeff[0] + 3) >> 3 sixteen times) otherwise, its outputs into position 0 of the
 *      sixteen luma blocks; then eob_adjust -- a luma block whose eob is 0 but whose Walsh DC is not 0 is still transformed --; then
 *      vp8_dequant_idct_add_y_block with the DC factor 1 and vp8_dequant_idct_add_uv_block: a block whose (adjusted) eob is above 1
 *      is dequantised from its LEVELS ((int16)(qcoeff * dequant), position 0 of luma the Walsh DC itself) and goes through
 *      vp8_short_idct4x4llm_c, any other adds ((int16)(position 0 * its factor) + 4) >> 3 to all sixteen pixels; clamped to 0..255.
 *
 * OUTPUTS, in the caller's device memory, each optional, at least one present; job i's at the pointer + i * its stride BYTES:
 *   coef    [mb_rows][mb_cols][25][16] of int16, 800 bytes a macroblock, position 4 v + u inside a block (v the vertical frequency):
 *           the reference's MACROBLOCKD.qcoeff[400] as it stands after step 4 -- Y 0..15, U 16..19, V 20..23, Y2 24.  p->stage
 *           selects VP8HIP_COEF_LEVELS (qcoeff) or VP8HIP_COEF_DEQUANT (dqcoeff).  A record layout for readers that walk macroblocks,
 *           not vp8hip_frames_coef_async's planes: block b, position 4 v + u here is that call's plane (Y: b < 16, U, V, Y2), block
 *           (4 my + b / 4, 4 mx + b % 4) (chroma: (2 my + (b & 3) / 2, 2 mx + (b & 1))), raster position 4 v + u -- and the IR's
 *           block (vp8_ir.h: column-major) is the transpose, entry 4 u + v.  Pointer and stride multiples of 16.
 *           vp8hip_quant_coef_size(ctx) = 800 * mb_rows * mb_cols.
 *   eob     [mb_rows][mb_cols][32] of uint8: the quantiser's eob of blocks 0..24 -- BEFORE eob_adjust --, entries 25..31 written as 0.
 *           Pointer and stride multiples of 4.  vp8hip_quant_eob_size(ctx) = 32 * mb_rows * mb_cols.
 *   stats   [popcount(p->planes)][mb_rows][mb_cols] of uint32 (pointer and stride multiples of 4), the planes in bit order:
 *             VP8HIP_QUANT_ERRY    vp8_mbblock_error_c(mb, 1): the sum over luma blocks, positions 1..15, of (coeff - dqcoeff)^2;
 *             VP8HIP_QUANT_ERRY2   vp8_block_error_c of block 24: all sixteen positions;
 *             VP8HIP_QUANT_ERRUV   vp8_mbuverror_c: blocks 16..23, all sixteen positions;
 *             VP8HIP_QUANT_EOBS    the sum of the 25 eobs;
 *             VP8HIP_QUANT_RECSSE  the sum over the macroblock's 384 pixels of (source - reconstruction)^2: this library's own
 *                                  figure, from which PSNR at the quantiser follows.
 *           The three errors are not 0 for identical pictures: vp8_short_fdct4x4_c of a zero block leaves 1 at position 1 (its
 *           rounding constant 14500 >> 12 = 3 in four rows, (12 + 7) >> 4), so ERRY is 16 and ERRUV 8 there, as in the reference.
 *           vp8hip_quant_stats_size(ctx, p) = 4 * popcount * mb_rows * mb_cols, 0 for planes == 0 or unknown bits.  p->planes is not
 *           read where stats is NULL, except for unknown bits.
 *   rec     the reconstruction of step 5 as packed I420 at the DISPLAY size, vp8hip_i420_size(w, h) bytes:
 *           vp8hip_frames_tfilter_async's dst layout.
 * Only what an output needs is computed: a call without rec and without VP8HIP_QUANT_RECSSE makes no inverse transform.
 *
 * The call is its neighbours: enqueued on the context's stream -- a later writer of a frame buffer runs behind it, an earlier
 * vp8hip_decode is seen --; nothing is converted, no raster pool is made and no device memory is added (the tables travel in the
 * arguments of the launches; a call of many jobs, or of many different qindex values, is cut into launches where those are full);
 * no frame buffer is written; only bytes inside an output's own [pointer + i * stride, + size) are written; no atomics: the same
 * bits in every run.  It returns -2 with nothing enqueued for n < 1; an fb or ref_fb out of range (ref_fb < 0 included); a qindex
 * outside 0..127 (p->qindex where job_qindex is NULL, else any of its n); a delta outside -15..15; an unknown quantizer, filter or
 * stage; a zero-bin term outside +-1048576; plane bits other than the five; stats with planes == 0; all four outputs NULL; a stride
 * below the size; a pointer or stride not aligned (mv: 2, coef: 16, eob: 4, stats: 4); an output or mv that is not device memory of
 * the context's device or that cannot hold n jobs; outputs that overlap each other or mv.
 *
 * vp8hip_quant_factors(qindex, delta, out): host only, no context, no GPU.  What the reference's vp8cx_init_quantizer computes with
 * sf.improved_quant on, for one qindex (0..127) and the five deltas (-15..15 each, the order above; NULL: all 0), for each of Y1, Y2
 * and UV: the dc and the ac value of quant, quant_shift, quant_fast, zbin, round and dequant, and the sixteen zrun_zbin_boost
 * values.  With d the dequant value -- vp8_dc_quant, vp8_dc2quant, vp8_dc_uv_quant, vp8_ac_yquant, vp8_ac2quant, vp8_ac_uv_quant:
 * vp8hip_dequant_factors' six --, l = floor(log2 d): quant = (int16)(1 + (1 << (16 + l)) / d - (1 << 16)), quant_shift = l,
 * quant_fast = (1 << 16) / d, zbin = ((qindex < 48 ? 84 : 80) * d + 64) >> 7, round = (48 * d) >> 7, and zrun_zbin_boost[i] =
 * (d * {0, 0, 8, 10, 12, 14, 16, 20, 24, 28, 32, 36, 40, 44, 44, 44}[i]) >> 7 with d the dc value at i == 0 and the ac value
 * elsewhere.  The call's plan uses it; a consumer of LEVELS that wants to requantise calls it too.  -2 for a NULL out or a value out
 * of range. */
#define VP8HIP_QUANT_REGULAR 0
#define VP8HIP_QUANT_FAST    1
#define VP8HIP_QUANT_ERRY    1   /* bit order = plane order */
#define VP8HIP_QUANT_ERRY2   2
#define VP8HIP_QUANT_ERRUV   4
#define VP8HIP_QUANT_EOBS    8
#define VP8HIP_QUANT_RECSSE  16
typedef struct vp8hip_quant_table {        /* [0] Y1, [1] Y2, [2] UV; [][0] dc, [][1] ac */
    int16_t quant[3][2], quant_shift[3][2], quant_fast[3][2], zbin[3][2], round[3][2], dequant[3][2];
    int16_t zrun_zbin_boost[3][16];
} vp8hip_quant_table;
typedef struct vp8hip_quant {
    int qindex;                /* 0..127; not read where job_qindex is given */
    int delta[5];              /* y1dc, y2dc, y2ac, uvdc, uvac: -15..15 */
    int quantizer;             /* VP8HIP_QUANT_REGULAR / _FAST */
    int filter;                /* VP8HIP_TFILTER_SIXTAP / _BILINEAR */
    int stage;                 /* of coef: VP8HIP_COEF_LEVELS / _DEQUANT */
    int zbin_over_quant, zbin_mode_boost, act_zbin_adj;   /* -1048576..1048576 each; the regular quantiser's */
    unsigned planes;           /* VP8HIP_QUANT_* bits of stats; may be 0 where stats is NULL */
    const uint8_t *job_qindex; /* host memory, n bytes, or NULL: p->qindex for every job */
} vp8hip_quant;
int  vp8hip_quant_factors(int qindex, const int delta[5], vp8hip_quant_table *out);
size_t vp8hip_quant_coef_size(const vp8hip_ctx *ctx);
size_t vp8hip_quant_eob_size(const vp8hip_ctx *ctx);
size_t vp8hip_quant_stats_size(const vp8hip_ctx *ctx, const vp8hip_quant *p);
int  vp8hip_frames_quant_async(vp8hip_ctx *ctx, const vp8hip_hist_job *jobs, int n, const vp8hip_quant *p, const void *mv, size_t mv_stride,
                               void *coef, size_t coef_stride, void *eob, size_t eob_stride, void *stats, size_t stats_stride, void *rec,
                               size_t rec_stride);
/* INTRA MODES AND LEVELS of key-frame macroblocks: the intra counterpart of vp8hip_frames_quant_async.  What the reference does per
 * macroblock of a key frame at real-time speed -- vp8_pick_intra_mode (vp8/encoder/pickinter.c) followed by the body of
 * vp8cx_encode_intra_macro_block (vp8/encoder/encodeframe.c) -- for every macroblock of any picture in the context's frame buffers,
 * bit for bit: the modes, the levels, the eobs, three figures of the decision and the reconstruction, in the caller's device
 * memory.  With it a stream can begin, and a scene cut can be coded, without leaving the device; writing the key frame's bytes from
 * these outputs is not part of it (it is vp8hip_frames_pack_key_async's, below).  NOT part of it either: vp8_rd_pick_intra_mode, the trellis (`optimize` 0), activity masking,
 * segmentation, a choice between intra and inter, the loop filter -- the reconstruction is the UNFILTERED one, the one intra
 * prediction reads -- and rec into a frame buffer.
 *
 * JOBS.  fb[i], i < n: the SOURCE picture of job i, a frame-buffer index; any order, repeats allowed, either form.  It is read
 * exactly as vp8hip_frames_quant_async reads its fb: the coded area A x B = 16 mb_cols x 16 mb_rows, S(F).
 * QUANTISER.  p->q: vp8hip_quant as it stands -- qindex / job_qindex, delta[5], quantizer, stage, the three zero-bin terms, the same
 * ranges and the same vp8hip_quant_factors; q.filter and q.planes are not read.
 * MODE DECISION.  All arithmetic is in `int`; the ranges keep it inside 31 bits.  p->rdmult 0..1000, p->rddiv 1..100 (the reference's:
 * vp8hip_intra_rd below), p->cost.mbmode_cost[5] (DC, V, H, TM, B_PRED) and p->cost.bmode_cost[above][left][mode], each 0..65535 (the
 * reference's: vp8hip_intra_costs below).  RDCOST(rate, dist) = ((128 + rate * rdmult) >> 8) + rddiv * dist.  p->bmode_last, 0..9:
 * the last sub-block mode tried.  The reference's picker tries B_DC_PRED .. B_HE_PRED only -- its loop bound, 3 --; 9 tries all
 * ten: the one place the call goes beyond the reference, a loop bound over the decoder's own predictors.  p->flags:
 * VP8HIP_INTRA_NO_BPRED leaves step 3 out.
 *
 * Per macroblock (r, c), in raster order's dependencies:
 *   0. NEIGHBOURS are the reconstruction (step 5) of macroblocks of the same job already coded, never loop-filtered.  Outside the
 *      picture the decoder's rules hold (vp8_setup_intra_recon, vp8_extend_mb_row): the row above the picture is 127 from column -1
 *      through A + 3; the column left of it is 129, so the top-left pixel of (r > 0, 0) is 129 and of (0, c) 127; the above-right four
 *      pixels of the last macroblock column in rows r > 0 are the last pixel of the line above, four times.  In B_PRED the
 *      above-right of the right-hand block column is the macroblock's own above-right row for all four block rows
 *      (vp8_intra_prediction_down_copy).
 *   1. CHROMA MODE (pick_intra_mbuv_mode): the squared error over U and V together of the predictions DC ((sum + (1 << (shift - 1)))
 *      >> shift, shift = 2 + up + left, 128 with neither), V (the row above), H (the left column), TM (clamp(L + A - TL)); the first
 *      strict minimum in that order wins.
 *   2. 16x16 LUMA MODE: for DC (shift = 3 + up + left), V, H, TM the decoder's prediction P; vp8_variance16x16_c against the source:
 *      variance = sse - ((unsigned)(sum * sum) >> 8); rd = RDCOST(mbmode_cost[mode], variance); the first strict minimum wins: its rd
 *      is error16x16, its sse best_sse.
 *   3. B_PRED (pick_intra4x4mby_modes): cost = mbmode_cost[B_PRED], dist = 0; for block b = 0..15 in raster order: the contexts A and
 *      L are the modes of the block above and of the block to the left -- inside the macroblock those just chosen, in a neighbour
 *      macroblock its sub-block modes or those its 16x16 mode implies (DC: B_DC, V: B_VE, H: B_HE, TM: B_TM), outside the picture
 *      B_DC --; for mode 0..bmode_last: vp8_intra4x4_predict, d = the 4x4 squared error, rd = RDCOST(bmode_cost[A][L][mode], d), the
 *      first strict minimum wins; the block is encoded as vp8_encode_intra4x4block does -- residual, vp8_short_fdct4x4_c, the
 *      quantiser over the Y1 factors on all sixteen positions (position 0 with the dc factors), vp8_short_idct4x4llm_c of dqcoeff
 *      where eob > 1, else vp8_dc_only_idct_add of dqcoeff[0], onto the prediction --, and its reconstruction is the neighbour of the
 *      blocks after it; cost += rate, dist += d; where dist > best_sse the macroblock breaks out and error4x4 is INT_MAX; after
 *      the sixteenth block error4x4 = RDCOST(cost, dist).  With VP8HIP_INTRA_NO_BPRED error4x4 is INT_MAX.
 *   4. B_PRED wins where error4x4 < error16x16.
 *   5. ENCODE.  B_PRED: step 3's levels and reconstruction; there is no Y2 block: block 24 is zero and eob[24] is 0.  Otherwise
 *      vp8_encode_intra16x16mby then vp8_inverse_transform_mby: vp8hip_frames_quant_async's steps 2-5 on the winner's prediction.
 *      Chroma in both cases: vp8_encode_intra16x16mbuv then vp8_dequant_idct_add_uv_block on step 1's prediction.
 *
 * OUTPUTS, all in the caller's device memory, each optional (NULL), at least one; job i's lies at pointer + i * stride:
 *   coef, eob, rec   vp8hip_frames_quant_async's layouts and size functions, unchanged.  For a B_PRED macroblock position 0 of the luma
 *           blocks IS coded and block 24 is zero.
 *   modes   [mb_rows][mb_cols][32] of uint8, vp8hip_intra_modes_size(ctx) = 32 * mb_rows * mb_cols; pointer and stride multiples of 4.
 *           [0] the y mode in vp8_ir.h's numbering (0..4); [1] the uv mode; [2] 1 where nothing is left to code (mb_is_skippable: with
 *           a Y2 block every luma eob < 2 and the nine others 0; B_PRED: all 24 zero); [3] 0; [4..19] the sixteen sub-block modes,
 *           the implied ones for a 16x16 mode; [20..31] 0.
 *   stats   uint32 planes [mb_rows][mb_cols], one per bit of p->planes in bit order; pointer and stride multiples of 4;
 *           vp8hip_intra_stats_size(ctx, p) = 4 * popcount * mb_rows * mb_cols, 0 for planes == 0 or unknown bits:
 *             VP8HIP_INTRA_RD16    error16x16;
 *             VP8HIP_INTRA_RD4     error4x4, 0x7FFFFFFF where broken out or not tried;
 *             VP8HIP_INTRA_RATE    what vp8_pick_intra_mode returns: the winner's rate;
 *             VP8HIP_INTRA_EOBS    the sum of the 25 eobs;
 *             VP8HIP_INTRA_RECSSE  the sum over the macroblock's 384 pixels of (source - reconstruction)^2.
 *
 * The call is its neighbours: enqueued on the context's stream; no device memory is added (tables and costs travel in the
 * arguments of the launches; a call of many jobs, or of more than four different qindex values, is cut into launches); no frame
 * buffer is written; only bytes inside an output's own range are written; no atomics: the same bits in every run.  It refuses no
 * size the context accepts.  -2 with nothing enqueued for n < 1; an fb out of range; a qindex outside 0..127; a delta outside
 * -15..15; an unknown quantizer or stage; a zero-bin term outside +-1048576; rdmult, rddiv, a cost or bmode_last out of range;
 * unknown flags or plane bits; stats with planes == 0; all five outputs NULL; a stride below the size; a pointer or stride not
 * aligned (coef: 16, eob, modes, stats: 4); an output that is not device memory of the context's device or cannot hold n jobs;
 * outputs that overlap.
 *
 * vp8hip_intra_costs(out): host only, no context, no GPU.  The reference's key-frame mbmode_cost[KEY_FRAME][DC, V, H, TM, B_PRED] and
 * bmode_costs[10][10][10] as vp8_init_mode_costs computes them: vp8_cost_tokens over vp8_kf_ymode_prob / vp8_kf_bmode_prob with
 * vp8_prob_cost.  -2 for a NULL out.
 * vp8hip_intra_rd(qindex, y1dc_delta, zbin_over_quant, &rdmult, &rddiv): host only.  vp8_initialize_rd_consts for one pass: Qvalue =
 * vp8_dc_quant(qindex, y1dc_delta), capped at 160; rdmult = (int)(2.70 * q * q) in double; for zbin_over_quant > 0, modq =
 * (int)(q * (1.0 + 0.0015625 * zbin_over_quant)) and rdmult = (int)(2.70 * modq * modq); above 1000, rddiv = 1 and rdmult /= 100,
 * else rddiv = 100.  Not the two-pass term.  -2 for a NULL pointer, a qindex outside 0..127 or a delta outside -15..15. */
#define VP8HIP_INTRA_NO_BPRED 1  /* flags */
#define VP8HIP_INTRA_RD16    1   /* bit order = plane order */
#define VP8HIP_INTRA_RD4     2
#define VP8HIP_INTRA_RATE    4
#define VP8HIP_INTRA_EOBS    8
#define VP8HIP_INTRA_RECSSE  16
typedef struct vp8hip_intra_cost {
    int mbmode_cost[5];        /* DC, V, H, TM, B_PRED: 0..65535 */
    int bmode_cost[10][10][10];/* [above][left][mode]: 0..65535 */
} vp8hip_intra_cost;
typedef struct vp8hip_intra {
    vp8hip_quant q;            /* the quantiser; filter and planes are not read */
    int rdmult, rddiv;         /* 0..1000, 1..100 */
    int bmode_last;            /* 0..9; the reference's is 3 */
    unsigned flags;            /* VP8HIP_INTRA_NO_BPRED */
    unsigned planes;           /* VP8HIP_INTRA_* bits of stats; may be 0 where stats is NULL */
    vp8hip_intra_cost cost;
} vp8hip_intra;
int  vp8hip_intra_costs(vp8hip_intra_cost *out);
int  vp8hip_intra_rd(int qindex, int y1dc_delta, int zbin_over_quant, int *rdmult, int *rddiv);
size_t vp8hip_intra_modes_size(const vp8hip_ctx *ctx);
size_t vp8hip_intra_stats_size(const vp8hip_ctx *ctx, const vp8hip_intra *p);
int  vp8hip_frames_intra_async(vp8hip_ctx *ctx, const int *fb, int n, const vp8hip_intra *p, void *coef, size_t coef_stride, void *eob,
                               size_t eob_stride, void *stats, size_t stats_stride, void *rec, size_t rec_stride, void *modes,
                               size_t modes_stride);
/* COMPRESSED INTER FRAMES from quantised levels and vectors: the entropy coder behind vp8hip_frames_quant_async.
 * vp8hip_frames_pack_async takes that call's mv and coef tensors as they stand and writes, per job, one complete compressed VP8
 * inter frame (RFC 6386) into the caller's device memory: the 3-byte frame tag, the first partition, the partition size table, 1 to
 * 8 token partitions.  Nothing but the frame header's few fields goes through the host; it reads no frame buffer and no IR slot;
 * jobs are simply 0 .. n - 1.  Key frames and intra macroblocks, SPLITMV, segmentation and loop-filter deltas, the trellis, rate
 * control, containers and chaining rec back in as the next reference are not part of it.  This call codes every frame with the
 * default probability tables; probability updates and adaptation to the frame's own counts are
 * vp8hip_frames_pack_adapt_async's, below.
 *
 * THE YARDSTICK for every byte is the stream writer of the test suite (tests/vp8_writer.py, write_inter_frame), written from RFC
 * 6386 and arbitrated by the real reference decoder.  A partition is flushed as its BoolEncoder.finish does: the bits of the byte in
 * the making, then three more bytes of `bottom`, four bytes in all.  The reference's vp8_stop_encode pads differently -- 32 times
 * put(0, 128) -- and decodes alike.
 *
 * INPUTS, device memory.  mv: job i's [2][mb_rows][mb_cols] of int16 at mv + i * mv_stride BYTES (multiples of 2), channel 0 = x,
 * 1 = y, in 1/8 pel -- vp8hip_frames_subpel_async's units --, NULL: (0, 0) everywhere.  coef: job i's LEVELS records
 * [mb_rows][mb_cols][25][16] of int16 at coef + i * coef_stride (multiples of 16), position 4 v + u, blocks Y 0..15, U 16..19,
 * V 20..23, Y2 24: vp8hip_frames_quant_async's layout with p->stage VP8HIP_COEF_LEVELS.  Position 0 of luma blocks 0..15 is NOT
 * coded and is not read: every macroblock here has a Y2 block, and frames_quant leaves the y1dc-quantised value there.  There is no
 * eob input: a block's end is the last non-zero zigzag step (0 1 4 8 5 2 3 6 9 12 13 10 7 11 14 15), from step 1 for luma and from
 * step 0 otherwise, so an inconsistent eob cannot make a wrong stream.  Any int16 is data, never an address.
 *
 * PARAMETERS (vp8hip_pack).  version 0..3, show_frame 0..1, filter_type 0..1, filter_level 0..63, sharpness 0..7; qindex 0..127
 * for every job, or job_qindex, a HOST pointer to n bytes copied at the call, as in vp8hip_quant; delta[5] = y1dc, y2dc, y2ac, uvdc,
 * uvac, each -15..15; ref_frame 1..3 (LAST, GOLDEN, ALTREF), that of every macroblock; refresh_last, refresh_golden, refresh_alt,
 * sign_bias_golden, sign_bias_alt 0..1; copy_buffer_to_gf, copy_buffer_to_arf 0..2 (coded only where the refresh flag is 0);
 * log2_parts 0..3; prob_skip_false, prob_intra, prob_last, prob_gf 1..255 (0 is refused).  Fixed, as in the writer: segmentation
 * off, mode_ref_lf_delta_enabled 0, refresh_entropy_probs 1, mb_no_coeff_skip 1, no coefficient, mode or vector probability update:
 * the frame is coded with the default tables.
 *
 * THE FIRST PARTITION.  The header, in write_inter_frame's order: segmentation_enabled (0), filter_type, filter_level (6 bits),
 * sharpness (3), mode_ref_lf_delta_enabled (0), log2_parts (2), qindex (7), the five deltas (a 0 flag, or 1, four magnitude bits and
 * the sign), refresh_golden, refresh_alt, copy_buffer_to_gf (2, if !refresh_golden), copy_buffer_to_arf (2, if !refresh_alt),
 * sign_bias_golden, sign_bias_alt, refresh_entropy_probs (1), refresh_last, 1056 "no update" flags at vp8_coef_update_probs,
 * mb_no_coeff_skip (1), prob_skip_false, prob_intra, prob_last, prob_gf (8 each), the two intra probability update flags (0), 38 "no
 * update" flags at vp8_mv_update_probs.  Then per macroblock in raster order:
 *   1. the skip flag at prob_skip_false: 1 exactly where the reference's mb_is_skippable(x, 1) says so -- no coded level in any of the
 *      25 blocks (luma position 0 not counting);
 *   2. 1 at prob_intra (inter), then ref_frame: 0 at prob_last for LAST, else 1 and ref_frame - 2 at prob_gf;
 *   3. the mode.  near[] and cnt[] are RFC 6386 18.3's (vp8_find_near_mvs) over the above, the left and the above-left macroblock,
 *      weights 2, 2, 1: a neighbour outside the picture counts as intra (skipped); one inside has the GIVEN vector; a non-zero vector
 *      that differs from near[k] opens near[++k] (the above one always does); cnt[k] or, for a zero vector, cnt[0] takes the weight.
 *      All neighbours share ref_frame, so no sign bias applies.  p[i] = vp8_mode_contexts[cnt[i]][i].  In this order:
 *        ZEROMV     if the vector is (0, 0): 0 at p[0].  Otherwise 1 at p[0]; then cnt[1] += 1 if cnt[3] and near[k] == near[1]; cnt[3]
 *                   = 0 (the SPLITMV count: always 0 here); near[1] and near[2] with their counts swap if cnt[2] > cnt[1];
 *        NEARESTMV  if the vector equals near[1] clamped: 0 at p[1].  Otherwise 1 at p[1];
 *        NEARMV     if it equals near[2] clamped: 0 at p[2].  Otherwise 1 at p[2];
 *        NEWMV      0 at p[3]; best = (cnt[1] >= cnt[0] ? near[1] : near[0]) clamped; then (v - best) / 2 per component, row first,
 *                   through vp8_default_mv_context as RFC 6386 section 17 codes a component (short form below 8, else the long
 *                   form: bits 0, 1, 2, then 9 .. 4, then bit 3 if the magnitude is above 15; the sign if it is not 0).
 *      "clamped": the row to [-(16 my << 3) - 128, (16 (mb_rows - 1 - my) << 3) + 128], the column likewise with mx and mb_cols:
 *      the 16-pixel margin.  A decoder derives the same four modes and the given vectors back.
 *
 * TOKENS.  A macroblock of row r goes into partition r % (1 << log2_parts); a skipped one codes nothing.  Order: Y2 (block 24, type
 * 1), the sixteen luma blocks from position 1 (type 0), four U, four V (type 2).  The context of a block is above + left "had a
 * coded level", across macroblocks, 0 outside the picture and for skipped macroblocks.  Per block from its first step: "not end of
 * block" (unless the step before coded a zero), the token tree of RFC 6386 13.2 with vp8_default_coef_probs[type][band][context]
 * -- the context of the next step is 0, 1 or 2 for a level of 0, +-1, more --, DCT_CAT1..6 with their extra bits (categories begin
 * at 5, 7, 11, 19, 35, 67), the sign at 128; "end of block" after the block's end unless that is step 15.
 *
 * OUTPUTS, device memory.  dst: job i's frame at dst + i * dst_stride; at most `cap` bytes are ever written there, cap <=
 * dst_stride, dst, cap and dst_stride multiples of 16.  info: job i's 16 uint32 at info + 64 i (a multiple of 4):
 *   [0] status   [1] frame bytes   [2] first partition bytes   [3..10] token partition bytes (0 for partitions the frame does not
 *   have)   [11] skipped macroblocks   [12..15] ZEROMV, NEARESTMV, NEARMV, NEWMV macroblocks
 * -- the counts are what a later call needs to choose prob_skip_false; vp8hip_frames_pack_adapt_async makes that choice itself.
 * Status bits:
 *   VP8HIP_PACK_OVERFLOW    the frame does not fit cap, or its first partition exceeds the tag's 19 bits (or a token partition the
 *                           size table's 24);
 *   VP8HIP_PACK_BAD_VECTOR  an odd component, or a NEWMV difference outside +-1023 coded units (the writer would clip it silently);
 *   VP8HIP_PACK_BAD_LEVEL   a coded |level| above 2114, the end of DCT_CAT6;
 *   VP8HIP_PACK_CLAMPS      informational: some NEWMV vector lies beyond mb_to_edge - (19 << 3) or + (18 << 3), where the decoder's
 *                           clamp_mv_to_umv_border would move it.  The frame is valid, but does not decode to frames_quant's rec,
 *                           which never clamps.
 * With any of the first three: info[1] = 0, the bytes inside [dst, dst + cap) are unspecified, no byte outside is touched and the
 * other jobs are unaffected.  With OVERFLOW alone info[2..10] are the sizes the partitions would have had (a first partition is
 * counted on even where it no longer fits), so 3 + [2] + 3 (parts - 1) + the sum of [3..10] is the cap that suffices.
 *
 * vp8hip_pack_bound(ctx, log2_parts): a cap that always suffices, a multiple of 16; 0 for a context without a size or log2_parts
 * outside 0..3.  A put shortens the coder's range from 128..255 to at least 1, so it is followed by at most 7 renormalisation
 * shifts: 7 bits.  A macroblock is at most 32 puts of the first partition (skip, inter, two for the reference, four for the mode, two
 * components of twelve) and 25 blocks of 16 tokens of 19 puts (7 of the tree, 11 extra bits, the sign) and an end-of-block: 28 and
 * 6672 bytes.  The bound is 3 + (VP8HIP_PACK_HEAD_MAX + 8 + 28 MBs) + 3 (parts - 1) + 6672 MBs + 4 parts, rounded up: loose -- real
 * frames are a hundredth of it --, so a caller that knows its content passes a smaller cap and watches OVERFLOW.
 *
 * vp8hip_pack_header(p, qindex, out): host only, no context, no GPU.  The header fields above through a C bool encoder up to where
 * the per-macroblock data begin: out->bytes[0 .. nbytes) are the bytes BoolEncoder has written by then and bottom, range, bit_count
 * its state; cache, pending and settled the same in the form the device coder continues from (bytes[settled] = cache is the last
 * byte that is not 0xFF -- a later carry lands there --, `pending` bytes of 0xFF follow it; cache -1: nbytes is 0).  The plan calls
 * it per distinct qindex of a call and hands state and bytes to the device: the mirror of vp8_parser_export_entropy.  -2 for a NULL
 * or a value out of range (p->job_qindex and p->qindex are not read: the qindex is the argument).
 *
 * The call is its neighbours: enqueued on the context's stream; the same bits in every run (integer atomics only).  Scratch -- 32
 * bytes a macroblock of plan records and the regions the partitions are coded into before their sizes are known, min(cap, bound of
 * the partition) each -- is the context's, the buffer vp8hip_frames_rgb_async keeps (vp8hip_rgb_scratch_bytes,
 * vp8hip_release_staging); a call is cut into groups of jobs so that it stays under 2 GB (one job at least) -- with the default cap
 * at a large size that is few jobs a group, another reason to pass a realistic cap.  It returns -2 with nothing enqueued for n < 1;
 * a parameter out of range; a NULL coef, dst or info; cap < 16, cap > dst_stride, a stride below the size (mv: 4 MBs, coef: 800
 * MBs); a pointer, cap or stride not aligned (mv 2, coef 16, dst 16, info 4); memory that is not device memory of the context's
 * device or cannot hold n jobs; dst or info overlapping each other, mv or coef. */
#define VP8HIP_PACK_OVERFLOW   1
#define VP8HIP_PACK_BAD_VECTOR 2
#define VP8HIP_PACK_BAD_LEVEL  4
#define VP8HIP_PACK_CLAMPS     8
#define VP8HIP_PACK_HEAD_MAX   64
typedef struct vp8hip_pack {
    int version, show_frame, filter_type, filter_level, sharpness;
    int qindex;                /* 0..127; not read where job_qindex is given */
    int delta[5];              /* y1dc, y2dc, y2ac, uvdc, uvac: -15..15 */
    int ref_frame;             /* 1 LAST, 2 GOLDEN, 3 ALTREF */
    int refresh_last, refresh_golden, refresh_alt, copy_buffer_to_gf, copy_buffer_to_arf, sign_bias_golden, sign_bias_alt;
    int log2_parts;            /* 0..3 */
    int prob_skip_false, prob_intra, prob_last, prob_gf;   /* 1..255 */
    const uint8_t *job_qindex; /* host memory, n bytes, or NULL: qindex for every job */
} vp8hip_pack;
typedef struct vp8hip_pack_head {
    uint32_t bottom, range, bit_count, nbytes;
    int32_t cache;
    uint32_t pending, settled, reserved;
    uint8_t bytes[VP8HIP_PACK_HEAD_MAX];
} vp8hip_pack_head;
size_t vp8hip_pack_bound(const vp8hip_ctx *ctx, int log2_parts);
int  vp8hip_pack_header(const vp8hip_pack *p, int qindex, vp8hip_pack_head *out);
int  vp8hip_frames_pack_async(vp8hip_ctx *ctx, int n, const vp8hip_pack *p, const void *mv, size_t mv_stride, const void *coef,
                              size_t coef_stride, void *dst, size_t dst_stride, size_t cap, void *info);
/* COMPRESSED INTER FRAMES WITH ADAPTED PROBABILITIES.  vp8hip_frames_pack_adapt_async is vp8hip_frames_pack_async -- the same
 * inputs, macroblock modes, token order, partitions, flush and statuses -- except that each frame carries probabilities fitted to
 * its own counts by the reference encoder's rules (vp8_update_coef_probs, vp8_write_mvprobs, the skip and reference counts),
 * coded into its header wherever an update pays for itself, and is coded with them.  Counting, the choice and the header's
 * probability section all happen on the device; vp8hip_frames_pack_async and its bytes are unchanged.
 *
 * vp8hip_pack_probs is a job's probability set, 1104 bytes: coef[4][8][3][11] (block type, band, context, tree node: RFC 6386
 * 13.4), mvc[2][19] (row, column: is_short, sign, short[7] -- vp8_small_mvtree's nodes --, bits[10]: RFC 6386 17.2) and 10
 * reserved bytes, written as 0 and never read.  vp8hip_pack_probs_default(out) fills the defaults (vp8_default_coef_probs,
 * vp8_default_mv_context) on the host; NULL does nothing.
 *
 * vp8hip_pack_adapt: flags, any of VP8HIP_ADAPT_COEF, _MV, _SKIP, _REF; refresh_entropy_probs 0..1, the header bit; probs_in,
 * DEVICE memory, job i's BASELINE set at probs_in + i * probs_in_stride (pointer and stride multiples of 16; a stride of 0: one set
 * for all jobs), or NULL: the defaults.  The baseline is what a decoder holds when the frame arrives.
 *
 * 1. COUNTS.  Over the macroblocks that are not skipped, the reference's coef_counts[type][band][ctx][token] (tokenize.c): every
 *    coded step of every block adds 1 at the block's type (luma 0 from step 1, Y2 1, chroma 2; type 3 stays zero), the step's band,
 *    the context the token coder would use (above + left for the block's first step, then 0, 1 or 2 for a level of 0, +-1, more)
 *    and its token: 0 for a zero, 1..4 for +-1..4, 5..10 for DCT_CAT1..6; the end of block adds 1 at token 11, with band and
 *    context of the step behind the block's end, unless the block ends at step 15.  A block without a coded level is one end of
 *    block at its first step.  Per component (row, then column) of every NEWMV macroblock, skipped or not, the coded difference
 *    d = (v - best) / 2 is reduced as write_component_probs does, x = |d|: is_short_ct[x >= 8]; sign_ct[d < 0] if x; for x < 8
 *    short_ct[x]; else bit_ct[k][(x >> k) & 1] for all ten k -- bit 3 too, though it is not always coded.
 * 2. THE CHOICE, in unsigned 32-bit integers as the reference's.  cost(c0, c1, p) = (c0 * C[p] + c1 * C[255 - p]) >> 8 with C =
 *    vp8_prob_cost (csrc/host/vp8_enc_tables.c).
 *    COEF: per context the branch counts of its 12 token counts down vp8_coef_tree -- node 0 (end of block | any other), 1 (zero |
 *    rest), 2 (one | rest), 3 (2..4 | categories), 4 (2 | 3, 4), 5 (3 | 4), 6 (CAT1, 2 | CAT3..6), 7 (CAT1 | CAT2), 8 (CAT3, 4 |
 *    CAT5, 6), 9 (CAT3 | CAT4), 10 (CAT5 | CAT6); the end-of-block branch thus includes tokens that follow a zero, as the
 *    reference's does.  newp = (c0 * 256 + (tot >> 1)) / tot with tot = c0 + c1, 0 becomes 1, above 255 becomes 255; tot 0: 128.  s
 *    = cost(c0, c1, oldp) - cost(c0, c1, newp) - (8 + ((C[255 - upd] - C[upd]) >> 8)) with oldp the baseline and upd
 *    vp8_coef_update_probs' entry; the probability is updated iff s > 0 (the reference's path without error resilience).
 *    MV: per component c0, c1 of probability 0 = is_short_ct, 1 = sign_ct, 2..8 the branches of short_ct down vp8_small_mvtree
 *    ((0..3 | 4..7), (0, 1 | 2, 3), (0 | 1), (2 | 3), (4, 5 | 6, 7), (4 | 5), (6 | 7)), 9 + k = bit_ct[k].  newp = ((c0 * 255) /
 *    tot) & 254, 0 becomes 1; with tot 0 it is the DEFAULT context's value, not the baseline's, as in the reference.  It is updated
 *    iff cost(c0, c1, oldp) - cost(c0, c1, newp) > 6 + ((C[255 - upd] - C[upd] + 128) >> 8), upd from vp8_mv_update_probs.
 *    SKIP: prob_skip_false = (macroblocks not skipped) * 256 / macroblocks, clipped to 1..255.
 *    REF: vp8_convert_rfct_to_prob for a frame whose macroblocks are all inter on p->ref_frame: prob_intra 1; prob_last 255 for
 *    LAST, else 1; prob_gf 128 for LAST, 255 for GOLDEN, 1 for ALTREF.
 *    Without its flag a part keeps the baseline -- p's values for skip and the reference probabilities -- and codes no update.
 *    The EFFECTIVE set is the baseline with this frame's updates applied.
 * 3. THE FRAME.  The header as vp8hip_frames_pack_async's with refresh_entropy_probs as given; each of the 1056 coefficient flags
 *    is 1 where the probability is updated and then followed by the new value in 8 bits; the four header probabilities are the
 *    chosen ones; each of the 38 vector flags likewise, followed by newp >> 1 in 7 bits (a decoder doubles it and turns 0 into 1:
 *    newp again).  Macroblocks and tokens are coded with the effective set and the chosen prob_skip_false.
 *
 * OUTPUTS.  dst, dst_stride, cap: as vp8hip_frames_pack_async's.  info: job i's 32 uint32 at info + 128 i: [0..15] as that call's;
 * [16] coefficient probabilities updated; [17] vector probabilities updated; [18] the prob_skip_false coded; [19] the sum of the
 * positive s modulo 2^32, the reference's estimate of the saving in bits; [20..31] 0.  counts: NULL, or job i's 1216 uint32 at counts + 4864 i
 * (a multiple of 4): the 1152 token counts [4][8][3][12], then per component (row, column) 32 branch counts: is_short_ct[2],
 * sign_ct[2], short_ct[8], bit_ct[10][2] -- for callers with a rule of their own.  probs_out: NULL, or job i's effective set at
 * probs_out + 1104 i (a multiple of 16): where refresh_entropy_probs is 1, the next frame's probs_in.  A job whose status has
 * BAD_VECTOR or BAD_LEVEL counts nothing: its counts are 0, its probs_out the baseline, info[16..19] 0.  With OVERFLOW alone all of
 * them are as defined.
 *
 * vp8hip_pack_adapt_bound(ctx, log2_parts): vp8hip_pack_bound plus the worst case of the probability section, derived the same
 * way: 1056 flags with 8 literal bits, 35 literal bits, 38 flags with 7 literal bits are 9843 puts of at most 7 bits, 8613 bytes,
 * rounded to 8624.  vp8hip_pack_header_prefix(p, qindex, refresh_entropy_probs, out): host only; the header through refresh_last,
 * where the probability section begins, in vp8hip_pack_head's form; -2 as vp8hip_pack_header, or for refresh_entropy_probs
 * outside 0..1.
 *
 * Stream, determinism (integer atomics only), scratch and its groups under 2 GB, and what is refused: as vp8hip_frames_pack_async,
 * with 8320 more bytes of scratch a job; also -2 for a NULL a, flags outside 0..15, refresh_entropy_probs outside 0..1, probs_in,
 * counts or probs_out that are misaligned, not device memory or too small for n jobs, a probs_in_stride between 1 and 1103, or
 * info, counts, probs_out or dst overlapping each other or an input. */
#define VP8HIP_ADAPT_COEF 1
#define VP8HIP_ADAPT_MV   2
#define VP8HIP_ADAPT_SKIP 4
#define VP8HIP_ADAPT_REF  8
typedef struct vp8hip_pack_probs {
    uint8_t coef[4][8][3][11];
    uint8_t mvc[2][19];
    uint8_t reserved[10];
} vp8hip_pack_probs;
typedef struct vp8hip_pack_adapt {
    int flags;                 /* VP8HIP_ADAPT_* */
    int refresh_entropy_probs; /* 0..1 */
    const void *probs_in;      /* device memory, or NULL: the defaults */
    size_t probs_in_stride;    /* 0: one set for all jobs */
} vp8hip_pack_adapt;
void vp8hip_pack_probs_default(vp8hip_pack_probs *out);
size_t vp8hip_pack_adapt_bound(const vp8hip_ctx *ctx, int log2_parts);
int  vp8hip_pack_header_prefix(const vp8hip_pack *p, int qindex, int refresh_entropy_probs, vp8hip_pack_head *out);
int  vp8hip_frames_pack_adapt_async(vp8hip_ctx *ctx, int n, const vp8hip_pack *p, const vp8hip_pack_adapt *a, const void *mv, size_t mv_stride,
                                    const void *coef, size_t coef_stride, void *dst, size_t dst_stride, size_t cap, void *info, void *counts,
                                    void *probs_out);
/* COMPRESSED KEY FRAMES from intra modes and levels: the entropy coder behind vp8hip_frames_intra_async, the key-frame counterpart
 * of vp8hip_frames_pack_async.  vp8hip_frames_pack_key_async takes that call's modes and coef tensors as they stand and writes, per
 * job, one complete compressed VP8 key frame into the caller's device memory, so that with frames_motion, frames_subpel,
 * frames_quant and frames_pack behind it every byte of a stream is made on the device.  It codes with the default probability
 * tables; probability adaptation for key frames, segmentation, loop-filter deltas, scaling bits other than 0, mb_no_coeff_skip 0,
 * rate control and a combined "encode a key frame" call are not part of it.
 *
 * THE YARDSTICK for every byte is tests/vp8_writer.py's write_key_frame for the same content with segmentation off,
 * mode_ref_lf_delta_enabled 0, refresh_entropy_probs 1, mb_no_coeff_skip 1 and no coefficient probability update (the writer fixes
 * show_frame to 1; here the tag carries the given bit), every partition flushed as BoolEncoder.finish does: exactly how
 * vp8hip_frames_pack_async is tied to write_inter_frame.
 *
 * INPUTS, device memory, vp8hip_frames_intra_async's outputs.  modes: job i's [mb_rows][mb_cols][32] of uint8 at modes + i *
 * modes_stride (multiples of 4; the stride at least 32 MBs): byte 0 the y mode (0..4: DC, V, H, TM, B_PRED), byte 1 the uv mode
 * (0..3), bytes 4..19 the sixteen sub-block modes (0..9: B_DC, B_TM, B_VE, B_HE, B_LD, B_RD, B_VR, B_VL, B_HD, B_HU), which are
 * read ONLY where the y mode is B_PRED: for a 16x16 mode the contexts its neighbours see are the implied ones (DC: B_DC, V: B_VE,
 * H: B_HE, TM: B_TM), derived from byte 0.  Bytes 2, 3 and 20..31 are not read.  coef: the LEVELS records [mb_rows][mb_cols][25][16]
 * of int16 as vp8hip_frames_pack_async takes them (multiples of 16).  There is no eob input: a block's end is its last non-zero
 * zigzag step.  Any byte or int16 is data, never an address: a mode out of range is caught before it indexes a table.
 *
 * PER MACROBLOCK.  has_y2 = the y mode is not B_PRED.  With a Y2 block the macroblock is vp8hip_frames_pack_async's: position 0 of
 * the sixteen luma blocks is not coded and not read, luma is block type 0 coded from step 1, Y2 type 1, chroma type 2.  Without:
 * block 24 is not read and not coded, the sixteen luma blocks are type 3 and coded from step 0.  The macroblock is skipped exactly
 * where no coded level is left -- in 25 blocks with a Y2 block, in 24 without; the flag is derived from the levels, never from
 * modes[2], so an inconsistent input cannot make a wrong stream.
 *
 * THE FIRST PARTITION.  The header, in write_key_frame's order: color_space, clamping_type, segmentation_enabled (0), filter_type,
 * filter_level (6 bits), sharpness (3), mode_ref_lf_delta_enabled (0), log2_parts (2), qindex (7), the five deltas (a 0 flag, or 1,
 * four magnitude bits and the sign), refresh_entropy_probs (1), 1056 "no update" flags at vp8_coef_update_probs, mb_no_coeff_skip
 * (1), prob_skip_false (8).  Then per macroblock in raster order: the skip flag at prob_skip_false; the y mode down
 * vp8_kf_ymode_tree (B_PRED "0", DC "100", V "101", H "110", TM "111") at {145, 156, 163, 128}; for B_PRED the sixteen sub-block
 * modes in raster order down vp8_bmode_tree at vp8_kf_bmode_prob[A][L], A and L the modes of the block above and to the left --
 * inside the macroblock its own, in a neighbour macroblock that one's sub-block or implied modes, outside the picture B_DC --; the
 * uv mode (DC "0", V "10", H "110", TM "111") at {142, 114, 183}.
 *
 * TOKENS.  Partition r % (1 << log2_parts); a skipped macroblock codes nothing.  Order: Y2 (where present), sixteen luma, four U,
 * four V; the tokens of a block as vp8hip_frames_pack_async codes them with vp8_default_coef_probs.  The context of a luma or
 * chroma block is above + left "had a coded level" across macroblocks, 0 outside the picture and for skipped macroblocks.  THE Y2
 * CONTEXT is not the neighbouring macroblock's: a B_PRED macroblock, skipped or not, leaves it untouched, so the above (left) Y2
 * context of a macroblock is that of the nearest macroblock above it in its column (left of it in its row) that has a Y2 block: 1
 * if that one's Y2 block had a coded level, 0 if it had none, was skipped, or there is none (the reference decoder's
 * vp8_reset_mb_tokens_context).
 *
 * THE FRAME.  The 3-byte tag -- bit 0 is 0, version (3 bits), show_frame, the first partition's size (19) --, 9d 01 2a, width and
 * height as 14 bits each with scale 0 -- the context's DISPLAY size --, the first partition, the size table, the token partitions.
 *
 * PARAMETERS (vp8hip_pack_key).  version 0..3, show_frame, color_space, clamping_type, filter_type 0..1, filter_level 0..63,
 * sharpness 0..7; qindex / job_qindex and delta[5] as vp8hip_pack's; log2_parts 0..3; prob_skip_false 1..255.
 *
 * OUTPUTS.  dst, dst_stride, cap: as vp8hip_frames_pack_async's.  info: job i's 16 uint32 at info + 64 i: [0] status, [1] frame
 * bytes, [2] first partition bytes, [3..10] token partition bytes, [11] skipped macroblocks, [12] B_PRED macroblocks, [13..15] 0.
 * Status: VP8HIP_PACK_OVERFLOW and VP8HIP_PACK_BAD_LEVEL as there -- luma position 0 of a B_PRED macroblock is a coded level, its
 * block 24 is none --, and VP8HIP_PACK_BAD_MODE: a y mode above 4, a uv mode above 3, or a sub-block mode above 9 that is read.
 * With any of the three: info[1] = 0, the bytes inside [dst, dst + cap) are unspecified, no byte outside is touched and the other
 * jobs are unaffected.  With OVERFLOW alone info[2..10] are the sizes the partitions would have had, so 10 + [2] + 3 (parts - 1) +
 * the sum of [3..10] is the cap that suffices.  With BAD_LEVEL or BAD_MODE [2..10] are unspecified; [11] and [12] are counted as
 * defined, a y mode above 4 counting as a 16x16 mode (it has a Y2 block and is no B_PRED macroblock).
 *
 * vp8hip_pack_key_bound(ctx, log2_parts): a cap that always suffices, a multiple of 16, derived as vp8hip_pack_bound: 7 bits a put.
 * The first partition of a macroblock is at most the skip flag, the B_PRED bit, sixteen sub-block modes at the longest path of
 * vp8_bmode_tree (B_HD, B_HU: seven puts) and three puts for the uv mode: 117 puts, 819 bits, 103 bytes (a 16x16 macroblock has
 * seven puts).  The tokens are 24 blocks from step 0 or 25 of which sixteen from step 1: within vp8hip_pack_bound's 6672 bytes.
 * The bound is 10 + (VP8HIP_PACK_HEAD_MAX + 8 + 103 MBs) + 3 (parts - 1) + 6672 MBs + 4 parts, rounded up.
 *
 * vp8hip_pack_key_header(p, qindex, out): host only, the mirror of vp8hip_pack_header: the key frame's header fields through the C
 * bool encoder up to where the per-macroblock data begin, in vp8hip_pack_head's form; -2 for a NULL or a value out of range.
 *
 * Stream, determinism, scratch (32 bytes a macroblock of records and the partitions' regions, in the buffer
 * vp8hip_frames_rgb_async keeps), groups of at most 1024 jobs, eight headers and 2 GB: as vp8hip_frames_pack_async.  It returns -2
 * with nothing enqueued for what that call refuses, `modes` treated as `coef` is: NULL, misaligned (4), a stride below 32 MBs, not
 * device memory of the context's device, too small for n jobs, or overlapping dst or info. */
#define VP8HIP_PACK_BAD_MODE 16
typedef struct vp8hip_pack_key {
    int version, show_frame, color_space, clamping_type, filter_type, filter_level, sharpness;
    int qindex;                /* 0..127; not read where job_qindex is given */
    int delta[5];              /* y1dc, y2dc, y2ac, uvdc, uvac: -15..15 */
    int log2_parts;            /* 0..3 */
    int prob_skip_false;       /* 1..255 */
    const uint8_t *job_qindex; /* host memory, n bytes, or NULL: qindex for every job */
} vp8hip_pack_key;
size_t vp8hip_pack_key_bound(const vp8hip_ctx *ctx, int log2_parts);
int  vp8hip_pack_key_header(const vp8hip_pack_key *p, int qindex, vp8hip_pack_head *out);
int  vp8hip_frames_pack_key_async(vp8hip_ctx *ctx, int n, const vp8hip_pack_key *p, const void *modes, size_t modes_stride, const void *coef,
                                  size_t coef_stride, void *dst, size_t dst_stride, size_t cap, void *info);
/* the HIP device the context runs on (a device of -1 at vp8hip_create resolved) */
int  vp8hip_device(const vp8hip_ctx *ctx);
/* A frame buffer has two forms on the device: the RASTER form (vp8ir_geom: the reference's YV12 layout, borders included), which
 * the small-launch kernels write and everything that reads pixels by coordinate reads (inter prediction, vp8hip_frame_download,
 * the post-processing filters), and the TILED form a large launch leaves (macroblock-window tiles: the form in which a lane of
 * vp8_keyframe_kernel can write whole 64-byte sectors).  The library converts a frame when something needs the form it is not in
 * -- never behind the caller's back after a launch -- and reads tiles where it can: the MD5 kernel of vp8hip_frames_fetch_async
 * walks them.  vp8hip_frames_to_raster asks for the raster form of `count` consecutive frame buffers explicitly (asynchronous, on
 * the context's stream; a no-op for frames that have it).  vp8hip_set_direct_download(ctx, 1): a batch download of tiled frames
 * into page-locked memory IS the tiled -> raster pass, a kernel writing the host buffer (the frames' raster form never exists in
 * HBM; what lands in the destination's border bytes is then undefined) -- faster than the copy engines on an otherwise idle
 * device, slower beside other kernels, hence off by default (VP8HIP_DIRECT_DOWNLOAD=1 sets the default).
 * INTER PREDICTION reads a reference frame in either form (round 5).  A large launch ONE of whose references exists only as tiles
 * -- streams decoded in lock step: every launch predicts from what the launch before left -- reads all its references as tiles
 * (vp8_inter_pred_tiles_kernel; borders are address clamps): no tiled -> raster pass runs, and a reference that exists only in
 * raster form (a golden frame a small launch decoded, an uploaded one) is given its tiled form once (vp8_retile_kernel) and keeps
 * both.  Any other launch -- every reference has a raster form already, or the launch is a small one -- reads the raster form.
 * vp8hip_set_pred_tiles(ctx, mode): 1 that rule (the default; VP8HIP_PRED_TILES sets it), 2 large launches always read tiles
 * (references without them are retiled), 0 never -- the three give the same frames, bit for bit.  Frames 16 pixels wide are always
 * read in raster form (a strip of the tile reader replicates one horizontal edge, and theirs reach past both). */
int  vp8hip_frames_to_raster(vp8hip_ctx *ctx, int first_fb, int count);
int  vp8hip_set_direct_download(vp8hip_ctx *ctx, int on);
int  vp8hip_set_pred_tiles(vp8hip_ctx *ctx, int mode);
/* Upload a whole frame buffer (frame_size bytes) -- tests and VP8_SET_REFERENCE. */
int  vp8hip_frame_upload(vp8hip_ctx *ctx, int fb, const uint8_t *buf);
int  vp8hip_frame_copy(vp8hip_ctx *ctx, int dst_fb, int src_fb);

/* Page-locked host memory for the caller's side of vp8hip_frame_download / vp8hip_frame_upload (a download into pageable
 * memory runs at a fraction of the PCIe rate).  The reference keeps its frame buffers in host memory it owns
 * (vp8_yv12_alloc_frame_buffer, vpx_scale/generic/yv12config.c:45-110); this is the host mirror's allocator. */
void *vp8hip_host_alloc(vp8hip_ctx *ctx, size_t bytes);
void  vp8hip_host_free(vp8hip_ctx *ctx, void *p);

/* Waits for the context's work.  Also reports (-1 + vp8hip_last_error) if a kernel of the cross-CU family gave up on
 * a row hand-over -- a defect, not an input error; the frames of that launch are invalid.  vp8hip_frame_download checks
 * the same. */
int  vp8hip_sync(vp8hip_ctx *ctx);
int  vp8hip_get_stats(vp8hip_ctx *ctx, vp8hip_stats *st);
/* Stats of an earlier launch: back = 0 the last vp8hip_decode call, 1 the one before, ... (up to 31).  Waits
 * for that launch only, so a caller can time a pipelined sequence and read the kernel times afterwards. */
int  vp8hip_get_stats_at(vp8hip_ctx *ctx, int back, vp8hip_stats *st);
/* The HIP stream (hipStream_t, as void*) the work of this context is enqueued on, so callers can bracket it with their own
 * events.  (vp8hip_join: rounds 1-3 ran a pass on a second stream that callers with work of their own had to join; there is
 * no such stream any more and the call does nothing.  A caller that reads frame buffers with kernels of its own asks for
 * their raster form first: vp8hip_frames_to_raster.) */
void *vp8hip_stream(vp8hip_ctx *ctx);
int  vp8hip_join(vp8hip_ctx *ctx);

/* ---- per-block test surface of the lane-per-row arithmetic (csrc/hip/vp8_lane_blocks.hip): the per-lane code the large-launch
 * kernels are made of, one block / macroblock per lane, on the current HIP device.  Each call is a launch and a synchronisation;
 * returns 0 or a negative error.  Counterparts in the reference: vp8_loop_filter_frame's per-macroblock calls
 * (vp8/common/loopfilter.c:259-299: vp8_loop_filter_{mbv,bv,mbh,bh}[_simple]), vp8_intra4x4_predict (reconintra4x4.c:16),
 * vp8_dequant_idct_add_c (dequantize.c:29). */
/* in / out: n x 400 bytes = rows and columns -4..15 of a luma macroblock (20 x 20); par: n x 8 bytes = mblim, blim, lim, hev_thr,
 * left edge filtered, inner edges filtered, top edge filtered, filter type (0 normal, 1 simple) */
int  vp8hip_lane_loop_filter_mbs(const uint8_t *in, uint8_t *out, const uint8_t *par, int n);
/* the chroma role of the same: in / out: n x 144 bytes = rows and columns -4..7 of a chroma macroblock (12 x 12); par: as above.
 * Two block rows, the first with the macroblock's top edge; simple-filter macroblocks are left alone (loopfilter.c:283-299). */
int  vp8hip_lane_loop_filter_chroma_mbs(const uint8_t *in, uint8_t *out, const uint8_t *par, int n);
/* one edge across each line: lines / out: n x 8 bytes = p3 p2 p1 p0 q0 q1 q2 q3, n even, lines 2i and 2i+1 share lane i;
 * par: n/2 x 8 bytes = sharpness (0..7), filter level (0..63), frame type (0 key, 1 inter), kind (0 macroblock edge, 1 inner
 * edge, 2 simple filter on the macroblock-edge limit, 3 simple filter on the inner-edge limit), edge filtered (0 no), 3 unused.
 * The limits are derived on the device (vp8_loop_filter_update_sharpness, loopfilter.c:66-96, and the hev threshold table). */
int  vp8hip_lane_loop_filter_lines(const uint8_t *lines, uint8_t *out, const uint8_t *par, int n);
/* the loop filter's clamp(f + 3 w) on 16-bit pairs against its exact value and its stepwise form, for all 2^32 pairs (f, w):
 * *mismatches = pairs where they differ; first_bad: nbad (<= 4096) records of 4 words = the low half's pair f << 16 | w, the
 * high half's, the one-instruction result, the stepwise result */
int  vp8hip_lane_add3w_sweep(uint64_t *mismatches, uint32_t *first_bad, int nbad);
/* mode: n B_PREDICTION_MODEs; ctx: n x 16 bytes = above[0..7], left[0..3], top_left, 3 bytes of padding; out: n x 16 bytes, row-major */
int  vp8hip_lane_intra4x4(const uint8_t *mode, const uint8_t *ctx, uint8_t *out, int n);
/* coef: n x 16 in IR order (column-major, vp8_ir.h); dq: n x (dc, ac); pred / out: n x 16 bytes, row-major */
int  vp8hip_lane_dequant_idct_add(const int16_t *coef, const int16_t *dq, const uint8_t *pred, uint8_t *out, int n);

#ifdef __cplusplus
}
#endif
#endif /* VP8HIP_H */
