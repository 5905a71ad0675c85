/* Driver of tests/golden/make_intra_fixtures.py: runs the REFERENCE's key-frame macroblock loop with the functions
 * oracle/_ref/libvpxref.so exports -- vp8_pick_intra_mode, vp8_encode_intra4x4mby, vp8_encode_intra16x16mby, vp8_encode_intra16x16mbuv,
 * vp8_dequant_idct_add_y_block_c / _uv_block_c, vp8_short_inv_walsh4x4_c / _1_c, vp8_init_mode_costs, vp8_initialize_rd_consts,
 * vp8cx_init_quantizer and vp8cx_mb_init_quantizer, the block pointer set-ups, vp8_setup_intra_recon and vp8_extend_mb_row -- on the
 * MACROBLOCK of a zeroed VP8_COMP and a bordered destination picture of our own.  What the reference keeps static or inline around
 * them is restated here in our words and guarded by the known answers of tests/test_intra_cpu.py: the macroblock loop of
 * encode_mb_row (pointers, up / left, the copy of the source block), the body of vp8cx_encode_intra_macro_block, the choice between
 * the two inverse Walsh transforms with eob_adjust (vp8_inverse_transform_mby) and mb_is_skippable.  error16x16 and error4x4 are
 * locals of vp8_pick_intra_mode and cannot be read, so both are made here a second time, BEFORE the picker runs: error16x16 from
 * vp8_build_intra_predictors_mby_c, vp8_variance16x16_c and the macroblock's own costs (the picker's 16x16 loop in our words),
 * error4x4 from vp8_intra_prediction_down_copy, vp8_intra4x4_predict_c, a 4x4 squared error, vp8_encode_intra4x4block and the
 * contexts of the blocks above and to the left (pick_intra4x4mby_modes, pick_intra4x4block, above_block_mode and left_block_mode
 * in our words).  The picker then does all of it again from the same neighbours -- whatever the chain here wrote inside the
 * macroblock it writes itself before it reads it --, and its rate, its modes and everything after them are recorded.  Built into a scratch directory by make_intra_fixtures.py; nothing of it is loaded by the tests. */
#include <stdlib.h>
#include <string.h>

#include "vpx_config.h"
#include "vpx_rtcd.h"
#include "vp8/encoder/onyx_int.h"
#include "vp8/common/entropymode.h"
#include "vp8/common/quant_common.h"
#include "vp8/common/setupintrarecon.h"
#include "vp8/common/extend.h"

void vp8cx_init_quantizer(VP8_COMP *cpi);
void vp8cx_mb_init_quantizer(VP8_COMP *cpi, MACROBLOCK *x, int ok_to_skip);
void vp8_init_mode_costs(VP8_COMP *c);
void vp8_initialize_rd_consts(VP8_COMP *cpi, int Qvalue);
void vp8_pick_intra_mode(VP8_COMP *cpi, MACROBLOCK *x, int *rate);
void vp8_encode_intra4x4mby(MACROBLOCK *mb);
void vp8_encode_intra16x16mby(MACROBLOCK *x);
void vp8_encode_intra16x16mbuv(MACROBLOCK *x);
void vp8_build_block_offsets(MACROBLOCK *x);
void vp8_setup_block_ptrs(MACROBLOCK *x);
void vp8_encode_intra4x4block(MACROBLOCK *x, int ib);

static int rd_cost(const MACROBLOCK *x, int rate, int dist) { return ((128 + rate * x->rdmult) >> 8) + x->rddiv * dist; }

/* the sub-block mode that position b of a neighbour macroblock gives as a context: its own, or the one its 16x16 mode implies */
static int context_mode(const MODE_INFO *mb, int b)
{
    switch (mb->mbmi.mode) {
    case B_PRED: return mb->bmi[b].as_mode;
    case V_PRED: return B_VE_PRED;
    case H_PRED: return B_HE_PRED;
    case TM_PRED: return B_TM_PRED;
    default: return B_DC_PRED;
    }
}

/* error4x4 of the macroblock at xd->mode_info_context, the picker's B_PRED chain in our words: INT_MAX where it breaks out */
static int chain_error4x4(MACROBLOCK *x, int best_sse)
{
    MACROBLOCKD *xd = &x->e_mbd;
    MODE_INFO *mi = xd->mode_info_context;
    int cost = x->mbmode_cost[KEY_FRAME][B_PRED], dist = 0;

    vp8_intra_prediction_down_copy(xd);
    for (int i = 0; i < 16; i++) {
        BLOCKD *b = &xd->block[i];
        const BLOCK *be = &x->block[i];
        const unsigned char *s = *be->base_src + be->src;
        unsigned char *p = b->predictor_base + b->predictor_offset;
        const int A = i < 4 ? context_mode(mi - xd->mode_info_stride, i + 12) : mi->bmi[i - 4].as_mode;
        const int L = (i & 3) == 0 ? context_mode(mi - 1, i + 3) : mi->bmi[i - 1].as_mode;
        int best = 0x7fffffff, best_mode = B_DC_PRED, best_rate = 0, best_d = 0;

        for (int mode = B_DC_PRED; mode <= B_HE_PRED; mode++) {
            const int rate = x->bmode_costs[A][L][mode];
            int d = 0, rd;

            vp8_intra4x4_predict_c(*b->base_dst + b->dst, b->dst_stride, mode, p, 16);
            for (int r = 0; r < 4; r++)
                for (int c = 0; c < 4; c++) d += (s[r * be->src_stride + c] - p[16 * r + c]) * (s[r * be->src_stride + c] - p[16 * r + c]);
            rd = rd_cost(x, rate, d);
            if (rd < best) best = rd, best_mode = mode, best_rate = rate, best_d = d;
        }
        mi->bmi[i].as_mode = b->bmi.as_mode = best_mode;
        vp8_encode_intra4x4block(x, i);
        cost += best_rate;
        dist += best_d;
        if (dist > best_sse) return 0x7fffffff;
    }
    return rd_cost(x, cost, dist);
}

static VP8_COMP *comp_for(int q, const int *deltas, int fast, const int *zb)
{
    VP8_COMP *cpi = calloc(1, sizeof *cpi);
    VP8_COMMON *cm;

    if (!cpi) return 0;
    cpi->mb.ss = calloc(8 * MAX_MVSEARCH_STEPS + 1, sizeof(search_site));     /* (the speed features lay their search sites out there) */
    if (!cpi->mb.ss) return 0;
    cm = &cpi->common;
    cm->frame_type = KEY_FRAME;
    cm->base_qindex = q;
    cm->y1dc_delta_q = deltas[0];
    cm->y2dc_delta_q = deltas[1];
    cm->y2ac_delta_q = deltas[2];
    cm->uvdc_delta_q = deltas[3];
    cm->uvac_delta_q = deltas[4];
    cpi->zbin_over_quant = zb[0];
    cpi->zbin_mode_boost = zb[1];
    cpi->mb.act_zbin_adj = zb[2];
    vp8_entropy_mode_init();                                          /* (the encodings the next call counts along) */
    vp8_init_mbmode_probs(cm);
    vp8_default_bmode_probs(cm->fc.bmode_prob);
    vp8_kf_default_bmode_probs(cm->kf_bmode_prob);
    vp8_initialize_rd_consts(cpi, vp8_dc_quant(q, deltas[0]));      /* (sets the speed features too: ours come after it) */
    cpi->sf.improved_quant = 1;
    vp8cx_init_quantizer(cpi);
    cpi->mb.e_mbd.frame_type = KEY_FRAME;
    cpi->mb.short_fdct4x4 = vp8_short_fdct4x4_c;
    cpi->mb.short_fdct8x4 = vp8_short_fdct8x4_c;
    cpi->mb.short_walsh4x4 = vp8_short_walsh4x4_c;
    cpi->mb.quantize_b = fast ? vp8_fast_quantize_b_c : vp8_regular_quantize_b_c;
    cpi->mb.quantize_b_pair = fast ? vp8_fast_quantize_b_pair_c : vp8_regular_quantize_b_pair_c;
    cpi->mb.optimize = 0;
    cpi->mb.rdmult = cpi->RDMULT;
    cpi->mb.rddiv = cpi->RDDIV;
    return cpi;
}

static void free_comp(VP8_COMP *cpi)
{
    free(cpi->mb.ss);
    free(cpi);
}

/* mb[5]: mbmode_cost[KEY_FRAME][DC, V, H, TM, B_PRED]; b[1000]: bmode_costs; rd[128][2]: RDMULT and RDDIV of every qindex */
int intra_ref_helpers(int *mb, int *b, int *rd)
{
    static const int none[5] = {0, 0, 0, 0, 0};

    for (int q = 0; q < 128; q++) {
        VP8_COMP *cpi = comp_for(q, none, 0, none);

        if (!cpi) return -1;
        rd[2 * q] = cpi->RDMULT;
        rd[2 * q + 1] = cpi->RDDIV;
        if (q == 0) {
            const int order[5] = {DC_PRED, V_PRED, H_PRED, TM_PRED, B_PRED};

            for (int i = 0; i < 5; i++) mb[i] = cpi->mb.mbmode_cost[KEY_FRAME][order[i]];
            memcpy(b, cpi->mb.bmode_costs, 1000 * sizeof(int));
        }
        free_comp(cpi);
    }
    return 0;
}

/* src: the three dense planes of the source picture (w x h, two of w/2 x h/2).  zb: zbin_over_quant, zbin_mode_boost, act_zbin_adj.
 * Per macroblock in raster order: modes[18] (y mode, uv mode, the sixteen sub-block modes: those chosen, or 255 for a 16x16 mode),
 * qcoeff[400], eobs[25], rate, skip, rd16 (error16x16), rd4 (error4x4); rdc[2]: RDMULT, RDDIV; rec: the reconstruction, dense like src.  Returns 0. */
int intra_ref_run(unsigned char *const *src, int w, int h, int q, const int *deltas, int fast, const int *zb, int *rdc, unsigned char *modes,
                  short *qcoeff, unsigned char *eobs, int *rate, unsigned char *skip, int *rd16, int *rd4, unsigned char *const *rec)
{
    const int cols = w / 16, rows = h / 16, cw = w / 2, ch = h / 2, border = 32, stride = w + 2 * border, cstride = stride / 2;
    VP8_COMP *cpi = comp_for(q, deltas, fast, zb);
    MACROBLOCK *x;
    MACROBLOCKD *xd;
    YV12_BUFFER_CONFIG dst;
    unsigned char *py = calloc(1, (size_t)stride * (h + 2 * border)), *pu = calloc(1, (size_t)cstride * (ch + border)),
                  *pv = calloc(1, (size_t)cstride * (ch + border));
    MODE_INFO *mip = calloc((size_t)(cols + 1) * (rows + 1), sizeof *mip);

    if (!cpi || !py || !pu || !pv || !mip) return -1;
    x = &cpi->mb;
    xd = &x->e_mbd;
    rdc[0] = cpi->RDMULT;
    rdc[1] = cpi->RDDIV;
    memset(&dst, 0, sizeof dst);
    dst.y_width = w, dst.y_height = h, dst.y_stride = stride, dst.uv_width = cw, dst.uv_height = ch, dst.uv_stride = cstride;
    dst.y_buffer = py + border * stride + border;
    dst.u_buffer = pu + (border / 2) * cstride + border / 2;
    dst.v_buffer = pv + (border / 2) * cstride + border / 2;
    vp8_setup_intra_recon(&dst);
    xd->dst = dst;
    xd->mode_info_stride = cols + 1;
    xd->mode_info_context = mip + cols + 1 + 1;
    x->src.y_stride = w, x->src.uv_stride = cw;
    vp8_setup_block_dptrs(xd);
    vp8_build_block_offsets(x);
    vp8_setup_block_ptrs(x);
    vp8cx_mb_init_quantizer(cpi, x, 0);
    for (int r = 0; r < rows; r++) {
        xd->up_available = r != 0;
        for (int c = 0; c < cols; c++) {
            const int m = r * cols + c;
            MODE_INFO *mi = xd->mode_info_context;
            char e[25];
            int sk = 1, rt = 0, best_sse = 0;

            xd->dst.y_buffer = dst.y_buffer + 16 * r * stride + 16 * c;
            xd->dst.u_buffer = dst.u_buffer + 8 * r * cstride + 8 * c;
            xd->dst.v_buffer = dst.v_buffer + 8 * r * cstride + 8 * c;
            xd->left_available = c != 0;
            x->src.y_buffer = src[0] + 16 * r * w + 16 * c;
            x->src.u_buffer = src[1] + 8 * r * cw + 8 * c;
            x->src.v_buffer = src[2] + 8 * r * cw + 8 * c;
            for (int i = 0; i < 16; i++) memcpy(x->thismb + 16 * i, x->src.y_buffer + i * w, 16);
            mi->mbmi.segment_id = 0;
            rd16[m] = 0x7fffffff;                                        /* the picker's 16x16 loop and its chain, for their figures alone */
            for (int mode = DC_PRED; mode <= TM_PRED; mode++) {
                unsigned int sse;
                int var, rd;

                mi->mbmi.mode = mode;
                vp8_build_intra_predictors_mby_c(xd);
                var = (int)vp8_variance16x16_c(x->thismb, 16, xd->predictor, 16, &sse);
                rd = rd_cost(x, x->mbmode_cost[KEY_FRAME][mode], var);
                if (rd16[m] > rd) rd16[m] = rd, best_sse = (int)sse;
            }
            rd4[m] = chain_error4x4(x, best_sse);
            /* the body of vp8cx_encode_intra_macro_block */
            vp8_pick_intra_mode(cpi, x, &rt);
            if (mi->mbmi.mode == B_PRED) vp8_encode_intra4x4mby(x);
            else vp8_encode_intra16x16mby(x);
            vp8_encode_intra16x16mbuv(x);
            if (mi->mbmi.mode == B_PRED) {                               /* no Y2 block: what lies there is the last macroblock's */
                memset(xd->qcoeff + 384, 0, 32);
                xd->eobs[24] = 0;
            }
            memcpy(qcoeff + 400 * m, xd->qcoeff, 800);
            memcpy(eobs + 25 * m, xd->eobs, 25);
            for (int i = 0; i < 25; i++)                                 /* mb_is_skippable */
                sk &= mi->mbmi.mode != B_PRED && i < 16 ? xd->eobs[i] < 2 : !xd->eobs[i];
            skip[m] = (unsigned char)sk;
            rate[m] = rt;
            modes[18 * m] = (unsigned char)mi->mbmi.mode;
            modes[18 * m + 1] = (unsigned char)mi->mbmi.uv_mode;
            for (int i = 0; i < 16; i++) modes[18 * m + 2 + i] = mi->mbmi.mode == B_PRED ? (unsigned char)mi->bmi[i].as_mode : 255;
            if (mi->mbmi.mode != B_PRED) {                               /* vp8_inverse_transform_mby */
                memcpy(e, xd->eobs, 25);
                if (e[24] > 1) vp8_short_inv_walsh4x4_c(xd->dqcoeff + 384, xd->qcoeff);
                else vp8_short_inv_walsh4x4_1_c(xd->dqcoeff + 384, xd->qcoeff);
                for (int i = 0; i < 16; i++)                             /* eob_adjust */
                    if (e[i] == 0 && xd->qcoeff[16 * i] != 0) e[i]++;
                vp8_dequant_idct_add_y_block_c(xd->qcoeff, xd->dequant_y1_dc, xd->dst.y_buffer, stride, e);
            }
            vp8_dequant_idct_add_uv_block_c(xd->qcoeff + 256, xd->dequant_uv, xd->dst.u_buffer, xd->dst.v_buffer, cstride, xd->eobs + 16);
            xd->mode_info_context++;
        }
        vp8_extend_mb_row(&dst, xd->dst.y_buffer + 16, xd->dst.u_buffer + 8, xd->dst.v_buffer + 8);
        xd->mode_info_context++;
    }
    for (int r = 0; r < h; r++) memcpy(rec[0] + r * w, dst.y_buffer + r * stride, w);
    for (int r = 0; r < ch; r++) {
        memcpy(rec[1] + r * cw, dst.u_buffer + r * cstride, cw);
        memcpy(rec[2] + r * cw, dst.v_buffer + r * cstride, cw);
    }
    free(mip);
    free(py);
    free(pu);
    free(pv);
    free_comp(cpi);
    return 0;
}
