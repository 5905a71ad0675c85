/* Driver of tests/golden/make_tfilter_fixtures.py: calls the REFERENCE's vp8_temporal_filter_apply_c (vp8/encoder/temporal_filter.c)
 * over predictions made by its vp8_sixtap_predict16x16_c / 8x8_c, vp8_bilinear_predict16x16_c / 8x8_c and vp8_copy_mem16x16_c /
 * 8x8_c, as oracle/_ref/libvpxref.so exports them, for every macroblock of a centre picture and its sources.  What the reference
 * keeps static around them is restated here in our words and guarded by the known answers of tests/test_tfilter_cpu.py: where a
 * vector puts the three blocks and which function predicts them, the weight of a source from its error, and the normalisation with
 * the table of 0x80000 / i.  The pictures arrive bordered by replicated pixels (pad luma, pad / 2 chroma; the caller makes them wide
 * enough for the case's largest vector plus the taps); the reference build is generic-gnu, so the functions read the picture
 * directly.  Built into a scratch directory by make_tfilter_fixtures.py; nothing of it is loaded by the tests. */
#include <string.h>

#include "vpx_config.h"
#include "vpx_rtcd.h"

typedef void (*predict_fn)(unsigned char *, int, int, int, unsigned char *, int);

/* the three predictions of one macroblock into pred[384]: luma at (row, col) in 1/8 pel, chroma at half of it (arithmetic shift) */
static void predictors(unsigned char *y, unsigned char *u, unsigned char *v, int stride, int row, int col, int bilinear, unsigned char *pred)
{
    const predict_fn p16 = bilinear ? vp8_bilinear_predict16x16_c : vp8_sixtap_predict16x16_c;
    const predict_fn p8 = bilinear ? vp8_bilinear_predict8x8_c : vp8_sixtap_predict8x8_c;
    int off;

    y += (row >> 3) * stride + (col >> 3);
    if ((row | col) & 7) p16(y, stride, col & 7, row & 7, pred, 16);
    else vp8_copy_mem16x16_c(y, stride, pred, 16);
    row >>= 1;
    col >>= 1;
    stride = (stride + 1) >> 1;
    off = (row >> 3) * stride + (col >> 3);
    if ((row | col) & 7) {
        p8(u + off, stride, col & 7, row & 7, pred + 256, 8);
        p8(v + off, stride, col & 7, row & 7, pred + 320, 8);
    } else {
        vp8_copy_mem8x8_c(u + off, stride, pred + 256, 8);
        vp8_copy_mem8x8_c(v + off, stride, pred + 320, 8);
    }
}

/* centre: the three bordered planes of the centre picture; src: 3 * count bordered planes (y, u, v of source 0, then of source 1 ...).
 * w x h: the coded luma size; pad: the luma border (even).  mv: NULL or int32 [count][2][rows][cols] (x, y) in 1/8 pel.  err: NULL or
 * int32 [count][rows][cols].  out: the three filtered planes, dense (w x h, then two of w/2 x h/2); cnt: the same geometry in
 * uint16.  Returns 0. */
int tfilter_ref_run(unsigned char *const *centre, unsigned char *const *src, int w, int h, int pad, int count, const int *mv, const int *err,
                    int strength, int bilinear, int thresh_low, int thresh_high, unsigned char *out, unsigned short *cnt)
{
    const int stride = w + 2 * pad, cstride = (stride + 1) >> 1, cpad = pad / 2, cols = w / 16, rows = h / 16, cw = w / 2, ch = h / 2;
    unsigned int fixed_divide[512];

    fixed_divide[0] = 0;
    for (int i = 1; i < 512; i++) fixed_divide[i] = 0x80000 / i;
    for (int my = 0; my < rows; my++)
        for (int mx = 0; mx < cols; mx++) {
            const int yo = (pad + 16 * my) * stride + pad + 16 * mx, co = (cpad + 8 * my) * cstride + cpad + 8 * mx;
            unsigned int acc[384];
            unsigned short n[384];
            unsigned char pred[384];

            memset(acc, 0, sizeof acc);
            memset(n, 0, sizeof n);
            for (int k = 0; k < count; k++) {
                const int e = err ? err[(k * rows + my) * cols + mx] : 0;
                const int weight = e < thresh_low ? 2 : e < thresh_high ? 1 : 0;
                const int col = mv ? mv[((k * 2 + 0) * rows + my) * cols + mx] : 0, row = mv ? mv[((k * 2 + 1) * rows + my) * cols + mx] : 0;

                if (!weight) continue;
                predictors(src[3 * k] + yo, src[3 * k + 1] + co, src[3 * k + 2] + co, stride, row, col, bilinear, pred);
                vp8_temporal_filter_apply_c(centre[0] + yo, stride, pred, 16, strength, weight, acc, n);
                vp8_temporal_filter_apply_c(centre[1] + co, cstride, pred + 256, 8, strength, weight, acc + 256, n + 256);
                vp8_temporal_filter_apply_c(centre[2] + co, cstride, pred + 320, 8, strength, weight, acc + 320, n + 320);
            }
            for (int i = 0; i < 384; i++) {
                unsigned int pval = acc[i] + (n[i] >> 1);
                size_t at;

                pval *= fixed_divide[n[i]];
                pval >>= 19;
                if (i < 256) at = (size_t)(16 * my + i / 16) * w + 16 * mx + i % 16;
                else at = (size_t)w * h + (size_t)(i >= 320) * cw * ch + (size_t)(8 * my + (i & 63) / 8) * cw + 8 * mx + (i & 7);
                out[at] = (unsigned char)pval;
                cnt[at] = n[i];
            }
        }
    return 0;
}
