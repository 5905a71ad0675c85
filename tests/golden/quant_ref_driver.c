/* Driver of tests/golden/make_quant_fixtures.py: runs the REFERENCE's inter 16x16 encode of every macroblock of a picture pair with
 * the functions oracle/_ref/libvpxref.so exports -- vp8_build_inter16x16_predictors_mb (with its own chroma vector; need_to_clamp_mvs
 * 0), vp8_subtract_mby_c / _mbuv_c, vp8_short_fdct8x4_c, vp8_short_walsh4x4_c, vp8_regular_quantize_b_c / vp8_fast_quantize_b_c on
 * BLOCK / BLOCKD structs filled from a vp8cx_init_quantizer run on a zeroed VP8_COMP with sf.improved_quant = 1, vp8_mbblock_error_c,
 * vp8_block_error_c, vp8_mbuverror_c, vp8_short_inv_walsh4x4_c / _1_c and vp8_dequant_idct_add_y_block_c / _uv_block_c.  What the
 * reference keeps static around them is restated here in our words and guarded by the known answers of tests/test_quant_cpu.py:
 * where the blocks of a macroblock lie in src_diff, build_dcblock, the three zero-bin extras, the choice between the two inverse
 * Walsh transforms and eob_adjust.  The reference picture arrives bordered by replicated pixels (pad luma, pad / 2 chroma; the
 * caller makes it wide enough for the case's largest vector plus the taps); the reference build is generic-gnu, so the functions
 * read the picture directly.  Built into a scratch directory by make_quant_fixtures.py; nothing of it is loaded by the tests. */
#include <stdlib.h>
#include <string.h>

#include "vpx_config.h"
#include "vpx_rtcd.h"
#include "vp8/encoder/onyx_int.h"
#include "vp8/common/reconinter.h"

int vp8_block_error_c(short *coeff, short *dqcoeff);
int vp8_mbblock_error_c(MACROBLOCK *mb, int dc);
int vp8_mbuverror_c(MACROBLOCK *mb);
void vp8cx_init_quantizer(VP8_COMP *cpi);

static VP8_COMP *comp_for(const int *deltas)
{
    VP8_COMP *cpi = calloc(1, sizeof *cpi);

    if (!cpi) return 0;
    cpi->sf.improved_quant = 1;
    cpi->common.y1dc_delta_q = deltas[0];
    cpi->common.y2dc_delta_q = deltas[1];
    cpi->common.y2ac_delta_q = deltas[2];
    cpi->common.uvdc_delta_q = deltas[3];
    cpi->common.uvac_delta_q = deltas[4];
    vp8cx_init_quantizer(cpi);
    return cpi;
}

/* out[84]: quant, quant_shift, quant_fast, zbin, round, dequant as [Y1, Y2, UV][dc, ac], then zrun_zbin_boost [Y1, Y2, UV][16] */
int quant_ref_factors(int q, const int *deltas, short *out)
{
    VP8_COMP *cpi = comp_for(deltas);

    if (!cpi) return -1;
    for (int k = 0; k < 2; k++) {
        short *o = out + k;
        o[0] = cpi->Y1quant[q][k], o[2] = cpi->Y2quant[q][k], o[4] = cpi->UVquant[q][k];
        o += 6;
        o[0] = cpi->Y1quant_shift[q][k], o[2] = cpi->Y2quant_shift[q][k], o[4] = cpi->UVquant_shift[q][k];
        o += 6;
        o[0] = cpi->Y1quant_fast[q][k], o[2] = cpi->Y2quant_fast[q][k], o[4] = cpi->UVquant_fast[q][k];
        o += 6;
        o[0] = cpi->Y1zbin[q][k], o[2] = cpi->Y2zbin[q][k], o[4] = cpi->UVzbin[q][k];
        o += 6;
        o[0] = cpi->Y1round[q][k], o[2] = cpi->Y2round[q][k], o[4] = cpi->UVround[q][k];
        o += 6;
        o[0] = cpi->common.Y1dequant[q][k], o[2] = cpi->common.Y2dequant[q][k], o[4] = cpi->common.UVdequant[q][k];
    }
    for (int i = 0; i < 16; i++) {
        out[36 + i] = cpi->zrun_zbin_boost_y1[q][i];
        out[52 + i] = cpi->zrun_zbin_boost_y2[q][i];
        out[68 + i] = cpi->zrun_zbin_boost_uv[q][i];
    }
    free(cpi);
    return 0;
}

/* src: the three dense planes of the source picture (w x h, two of w/2 x h/2); ref: the three bordered planes of the reference
 * picture; pad: its luma border (even).  mv: NULL or int32 [2][rows][cols] (x, y) in 1/8 pel, inside int16 and not +-32767 / -32768.
 * zb: zbin_over_quant, zbin_mode_boost, act_zbin_adj.  Per macroblock in raster order: qcoeff[400], dqcoeff[400], eobs[25] (the
 * quantiser's), err[3] (mbblock_error(1), block_error of block 24, mbuverror); rec: the reconstruction, dense like src.  Returns 0. */
int quant_ref_run(unsigned char *const *src, unsigned char *const *ref, int w, int h, int pad, const int *mv, int q, const int *deltas, int fast,
                  int bilinear, const int *zb, short *qcoeff, short *dqcoeff, unsigned char *eobs, int *err, unsigned char *const *rec)
{
    const int stride = w + 2 * pad, cstride = stride >> 1, cpad = pad / 2, cols = w / 16, rows = h / 16, cw = w / 2;
    VP8_COMP *cpi = comp_for(deltas);
    MACROBLOCK *x = calloc(1, sizeof *x);
    MACROBLOCKD *xd = &x->e_mbd;
    MODE_INFO mi;
    const int zsum = zb[0] + zb[1] + zb[2], zsum2 = zb[0] / 2 + zb[1] + zb[2];

    if (!cpi || !x) return -1;
    memset(&mi, 0, sizeof mi);
    mi.mbmi.mode = NEWMV;
    mi.mbmi.ref_frame = LAST_FRAME;
    xd->mode_info_context = &mi;
    xd->fullpixel_mask = 0xffffffff;
    xd->subpixel_predict16x16 = bilinear ? vp8_bilinear_predict16x16_c : vp8_sixtap_predict16x16_c;
    xd->subpixel_predict8x8 = bilinear ? vp8_bilinear_predict8x8_c : vp8_sixtap_predict8x8_c;
    xd->block[0].pre_stride = stride;
    xd->dequant_y1_dc[0] = 1;
    xd->dequant_y1[0] = cpi->common.Y1dequant[q][0];
    xd->dequant_y2[0] = cpi->common.Y2dequant[q][0];
    xd->dequant_uv[0] = cpi->common.UVdequant[q][0];
    for (int i = 1; i < 16; i++) {
        xd->dequant_y1_dc[i] = xd->dequant_y1[i] = cpi->common.Y1dequant[q][1];
        xd->dequant_y2[i] = cpi->common.Y2dequant[q][1];
        xd->dequant_uv[i] = cpi->common.UVdequant[q][1];
    }
    for (int i = 0; i < 25; i++) {
        BLOCK *b = &x->block[i];
        BLOCKD *d = &xd->block[i];

        b->coeff = x->coeff + 16 * i;
        d->qcoeff_base = xd->qcoeff;
        d->dqcoeff_base = xd->dqcoeff;
        d->qcoeff_offset = d->dqcoeff_offset = 16 * i;
        d->eob = &xd->eobs[i];
        if (i < 16) {
            b->quant = cpi->Y1quant[q], b->quant_fast = cpi->Y1quant_fast[q], b->quant_shift = cpi->Y1quant_shift[q];
            b->zbin = cpi->Y1zbin[q], b->round = cpi->Y1round[q], b->zrun_zbin_boost = cpi->zrun_zbin_boost_y1[q];
            b->zbin_extra = (short)((cpi->common.Y1dequant[q][1] * zsum) >> 7);              /* ZBIN_EXTRA_Y */
            d->dequant = xd->dequant_y1;
        } else if (i < 24) {
            b->quant = cpi->UVquant[q], b->quant_fast = cpi->UVquant_fast[q], b->quant_shift = cpi->UVquant_shift[q];
            b->zbin = cpi->UVzbin[q], b->round = cpi->UVround[q], b->zrun_zbin_boost = cpi->zrun_zbin_boost_uv[q];
            b->zbin_extra = (short)((cpi->common.UVdequant[q][1] * zsum) >> 7);              /* ZBIN_EXTRA_UV */
            d->dequant = xd->dequant_uv;
        } else {
            b->quant = cpi->Y2quant[q], b->quant_fast = cpi->Y2quant_fast[q], b->quant_shift = cpi->Y2quant_shift[q];
            b->zbin = cpi->Y2zbin[q], b->round = cpi->Y2round[q], b->zrun_zbin_boost = cpi->zrun_zbin_boost_y2[q];
            b->zbin_extra = (short)((cpi->common.Y2dequant[q][1] * zsum2) >> 7);             /* ZBIN_EXTRA_Y2 */
            d->dequant = xd->dequant_y2;
        }
    }
    for (int my = 0; my < rows; my++)
        for (int mx = 0; mx < cols; mx++) {
            const int m = my * cols + mx;
            unsigned char pred[384];
            char e[25];

            xd->pre.y_buffer = ref[0] + (pad + 16 * my) * stride + pad + 16 * mx;
            xd->pre.u_buffer = ref[1] + (cpad + 8 * my) * cstride + cpad + 8 * mx;
            xd->pre.v_buffer = ref[2] + (cpad + 8 * my) * cstride + cpad + 8 * mx;
            mi.mbmi.mv.as_mv.col = mv ? mv[m] : 0;
            mi.mbmi.mv.as_mv.row = mv ? mv[rows * cols + m] : 0;
            mi.mbmi.need_to_clamp_mvs = 0;
            vp8_build_inter16x16_predictors_mb(xd, pred, pred + 256, pred + 320, 16, 8);
            vp8_subtract_mby_c(x->src_diff, src[0] + 16 * my * w + 16 * mx, w, pred, 16);
            vp8_subtract_mbuv_c(x->src_diff, src[1] + 8 * my * cw + 8 * mx, src[2] + 8 * my * cw + 8 * mx, cw, pred + 256, pred + 320, 8);
            /* transform_mb for a 16x16 mode: block i of luma lies at row 4 (i >> 2), column 4 (i & 3) of the 16-wide residual, a
             * chroma block of plane p at row 4 (j >> 1), column 4 (j & 1) of its 8-wide one */
            for (int i = 0; i < 16; i += 2) vp8_short_fdct8x4_c(x->src_diff + 64 * (i >> 2) + 4 * (i & 3), x->coeff + 16 * i, 32);
            for (int i = 0; i < 16; i++) x->src_diff[384 + i] = x->coeff[16 * i];            /* build_dcblock */
            for (int i = 16; i < 24; i += 2) {
                const int j = (i - 16) & 3;
                vp8_short_fdct8x4_c(x->src_diff + 256 + 64 * (i >= 20) + 32 * (j >> 1) + 4 * (j & 1), x->coeff + 16 * i, 16);
            }
            vp8_short_walsh4x4_c(x->src_diff + 384, x->coeff + 384, 8);
            for (int i = 0; i < 25; i++) {
                if (fast) vp8_fast_quantize_b_c(&x->block[i], &xd->block[i]);
                else vp8_regular_quantize_b_c(&x->block[i], &xd->block[i]);
            }
            memcpy(qcoeff + 400 * m, xd->qcoeff, 800);
            memcpy(dqcoeff + 400 * m, xd->dqcoeff, 800);
            memcpy(eobs + 25 * m, xd->eobs, 25);
            err[3 * m] = vp8_mbblock_error_c(x, 1);
            err[3 * m + 1] = vp8_block_error_c(x->coeff + 384, xd->dqcoeff + 384);
            err[3 * m + 2] = vp8_mbuverror_c(x);
            /* vp8_inverse_transform_mby, then the chroma blocks, on the prediction */
            memcpy(e, xd->eobs, 25);
            if (e[24] > 1) vp8_short_inv_walsh4x4_c(xd->dqcoeff + 384, xd->qcoeff);
            else vp8_short_inv_walsh4x4_1_c(xd->dqcoeff + 384, xd->qcoeff);
            for (int i = 0; i < 16; i++)                                                     /* eob_adjust */
                if (e[i] == 0 && xd->qcoeff[16 * i] != 0) e[i]++;
            vp8_dequant_idct_add_y_block_c(xd->qcoeff, xd->dequant_y1_dc, pred, 16, e);
            vp8_dequant_idct_add_uv_block_c(xd->qcoeff + 256, xd->dequant_uv, pred + 256, pred + 320, 8, e + 16);
            for (int r = 0; r < 16; r++) memcpy(rec[0] + (16 * my + r) * w + 16 * mx, pred + 16 * r, 16);
            for (int r = 0; r < 8; r++) {
                memcpy(rec[1] + (8 * my + r) * cw + 8 * mx, pred + 256 + 8 * r, 8);
                memcpy(rec[2] + (8 * my + r) * cw + 8 * mx, pred + 320 + 8 * r, 8);
            }
        }
    free(x);
    free(cpi);
    return 0;
}
