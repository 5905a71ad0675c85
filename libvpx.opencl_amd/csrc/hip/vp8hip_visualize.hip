// vp8hip_visualize (include/vp8hip.h): the host entry point of the decoder's debug overlays; the kernels are in vp8_visualize.hip.
#include "vp8hip_ctx.hip.h"

// vp8_visualize.hip
void vp8vis_text(hipStream_t st, uint8_t *fb, int frame_size, const DevGeom &g, const vp8ir_mbx *mbx, const char *str, int len,
                 int mode, int key_frame);
void vp8vis_mvs(hipStream_t st, uint8_t *fb, int frame_size, const DevGeom &g, const vp8ir_mbx *mbx, const vp8ir_mv *mvs, int mask);
void vp8vis_colours(hipStream_t st, uint8_t *fb, const DevGeom &g, const vp8ir_mbx *mbx, int blk_modes, int mb_mask, int b_mask,
                    int ref_mask);

#define VIS_TEXT_MAX 512        // bytes of staging per string (the reference formats into char[512])

// The phases of vp8_post_proc_frame's CONFIG_POSTPROC_VISUALIZER part (vp8/common/postproc.c:1007-1362), in its order, on the
// context's stream: text, motion vectors, block-mode colours, reference-frame colours.
extern "C" int vp8hip_visualize(vp8hip_ctx *c, int fb, int ir_slot, const vp8hip_vis *v)
{
    const int nfb = c ? (int)c->fb.size() : 0, nsl = c ? (int)c->slots.size() : 0;
    if (!c || !v || fb < 0 || fb >= nfb || ir_slot < 0 || ir_slot >= nsl)
        return fail(c, -2, "vp8hip_visualize: bad arguments");
    const unsigned flags = v->flags;
    const bool info = (flags & VP8HIP_VIS_TXT_FRAME_INFO) && v->frame_info, rate = (flags & VP8HIP_VIS_TXT_RATE_INFO) && v->rate_info;
    const size_t info_len = info ? strlen(v->frame_info) : 0, rate_len = rate ? strlen(v->rate_info) : 0;
    if (info_len >= VIS_TEXT_MAX || rate_len >= VIS_TEXT_MAX)
        return fail(c, -2, "vp8hip_visualize: strings are limited to %d characters", VIS_TEXT_MAX - 1);
    const Slot &s = c->slots[(size_t)ir_slot];
    const bool key = s.hdr_copy.frame_type == 0;
    const bool mb_text = flags & (VP8HIP_VIS_TXT_MBLK_MODES | VP8HIP_VIS_TXT_DC_DIFF);
    const bool mvs = (flags & VP8HIP_VIS_DRAW_MV) && v->mv_mask && !key;      // (key frames have no vectors)
    const bool blk = (flags & VP8HIP_VIS_CLR_BLK_MODES) && (v->mb_modes_mask || v->b_modes_mask);
    const bool ref = (flags & VP8HIP_VIS_CLR_FRM_REF_BLKS) && v->ref_frame_mask;
    if (!info && !rate && !mb_text && !mvs && !blk && !ref) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    if (vp8hip_raster_pool(c) || vp8hip_need_raster(c, fb, 1)) return -1;
    c->fb_state[(size_t)fb] = FB_RASTER;                 // (the tiled form, if any, no longer holds the picture)
    if (c->d2h_count) { HIPCHK(c, hipEventSynchronize(c->ev_d2h_done)); c->d2h_count = 0; }   // a batch download may be reading fb
    const char *d_info = nullptr, *d_rate = nullptr;
    if (info || rate) {
        // the strings go through a pinned copy of our own, so that the caller's may go away when the call returns
        HIPCHK(c, c->d_vis.grow(2 * VIS_TEXT_MAX));
        HIPCHK(c, c->h_vis.grow(2 * VIS_TEXT_MAX));
        if (c->ev_vis) HIPCHK(c, hipEventSynchronize(c->ev_vis));  // the previous call's copy has left the pinned staging
        else HIPCHK(c, c->ev_vis.ensure());
        if (info) memcpy(c->h_vis, v->frame_info, info_len);
        if (rate) memcpy(c->h_vis + VIS_TEXT_MAX, v->rate_info, rate_len);
        HIPCHK(c, hipMemcpyAsync(c->d_vis, c->h_vis, 2 * VIS_TEXT_MAX, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipEventRecord(c->ev_vis, c->stream));
        d_info = c->d_vis;
        d_rate = c->d_vis + VIS_TEXT_MAX;
    }
    uint8_t *buf = c->fb[(size_t)fb];
    const int frame_size = c->geom.frame_size;
    if (info) vp8vis_text(c->stream, buf, frame_size, c->dg, s.d_mbx, d_info, (int)info_len, 0, key);
    if (flags & VP8HIP_VIS_TXT_MBLK_MODES) vp8vis_text(c->stream, buf, frame_size, c->dg, s.d_mbx, nullptr, 0, 1, key);
    if (flags & VP8HIP_VIS_TXT_DC_DIFF) vp8vis_text(c->stream, buf, frame_size, c->dg, s.d_mbx, nullptr, 0, 2, key);
    if (rate) vp8vis_text(c->stream, buf, frame_size, c->dg, s.d_mbx, d_rate, (int)rate_len, 0, key);
    if (mvs) vp8vis_mvs(c->stream, buf, frame_size, c->dg, s.d_mbx, s.d_mvs, v->mv_mask);
    if (blk || ref)
        vp8vis_colours(c->stream, buf, c->dg, s.d_mbx, blk, blk ? v->mb_modes_mask : 0, blk ? v->b_modes_mask : 0, ref ? v->ref_frame_mask : 0);
    HIPCHK(c, hipGetLastError());
    return 0;
}
