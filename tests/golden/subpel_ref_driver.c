/* Driver of tests/golden/make_subpel_fixtures.py: calls the REFERENCE's vp8_find_best_sub_pixel_step and
 * vp8_find_best_half_pixel_step (vp8/encoder/mcomp.c) over vp8_variance16x16_c, vp8_sub_pixel_variance16x16_c and the three
 * vp8_variance_halfpixvar16x16_*_c, as oracle/_ref/libvpxref.so exports them, for every macroblock of a picture pair.  It fills the
 * few fields of MACROBLOCK / BLOCK / BLOCKD / vp8_variance_fn_ptr_t the two functions read and records what came back.  The pictures
 * arrive bordered by 32 replicated pixels (the reference's border extension), made by the caller; the reference build is
 * generic-gnu, so the functions read the picture directly.  Built into a scratch directory by make_subpel_fixtures.py; nothing of it
 * is loaded by the tests. */
#include <limits.h>
#include <stdlib.h>
#include <string.h>

#include "vpx_config.h"
#include "vpx_rtcd.h"
#include "vp8/encoder/block.h"
#include "vp8/encoder/variance.h"

#define BORDER 32              /* VP8BORDERINPIXELS */
#define RESULTS 6              /* per macroblock: x, y (1/8 pel), the return value, *distortion, *sse1, the variance at the start */

typedef int (*step_fn)(MACROBLOCK *, BLOCK *, BLOCKD *, int_mv *, int_mv *, int, const vp8_variance_fn_ptr_t *, int *[2], int *, unsigned int *);
extern int vp8_find_best_sub_pixel_step(MACROBLOCK *, BLOCK *, BLOCKD *, int_mv *, int_mv *, int, const vp8_variance_fn_ptr_t *, int *[2], int *,
                                        unsigned int *);
extern int vp8_find_best_half_pixel_step(MACROBLOCK *, BLOCK *, BLOCKD *, int_mv *, int_mv *, int, const vp8_variance_fn_ptr_t *, int *[2], int *,
                                         unsigned int *);

/* src / ref: pictures of (w + 64) x (h + 64) bytes, the coded area at (32, 32).  start: int32 [2][rows][cols] (x, y) in whole pixels,
 * inside the UMV bounds.  rvec: int32 [2][rows][cols] (x, y) in 1/8 pel.  cost: NULL or int32 [2][2 R + 1].  out: int32
 * [rows * cols][RESULTS].  Returns 0. */
int subpel_ref_run(const unsigned char *src, const unsigned char *ref, int w, int h, const int *start, const int *rvec, const int *cost, int R,
                   int error_per_bit, int precision, int *out)
{
    const int stride = w + 2 * BORDER, cols = w / 16, rows = h / 16;
    MACROBLOCK *x = calloc(1, sizeof *x);
    BLOCK b;
    BLOCKD bd;
    vp8_variance_fn_ptr_t fn;
    static int zeros[2][2 * 1023 + 1];
    int *mvcost[2] = {zeros[0] + 1023, zeros[1] + 1023};
    unsigned char *src_base = (unsigned char *)src + BORDER * stride + BORDER, *ref_base = (unsigned char *)ref + BORDER * stride + BORDER;
    const step_fn step = precision == 2 ? vp8_find_best_half_pixel_step : vp8_find_best_sub_pixel_step;

    memset(&b, 0, sizeof b);
    memset(&bd, 0, sizeof bd);
    memset(&fn, 0, sizeof fn);
    fn.vf = vp8_variance16x16_c;
    fn.svf = vp8_sub_pixel_variance16x16_c;
    fn.svf_halfpix_h = vp8_variance_halfpixvar16x16_h_c;
    fn.svf_halfpix_v = vp8_variance_halfpixvar16x16_v_c;
    fn.svf_halfpix_hv = vp8_variance_halfpixvar16x16_hv_c;
    if (cost) {
        mvcost[0] = (int *)cost + R;
        mvcost[1] = (int *)cost + (2 * R + 1) + R;
    }
    for (int my = 0; my < rows; my++)
        for (int mx = 0; mx < cols; mx++) {
            int *o = out + (my * cols + mx) * RESULTS;
            const int k = my * cols + mx;
            int_mv best, ref_mv;
            int distortion = 0;
            unsigned int sse = 0, sse0 = 0;
            b.base_src = &src_base;
            b.src = my * 16 * stride + mx * 16;
            b.src_stride = stride;
            bd.base_pre = &ref_base;
            bd.pre = my * 16 * stride + mx * 16;
            bd.pre_stride = stride;
            best.as_mv.col = (short)start[k];
            best.as_mv.row = (short)start[rows * cols + k];
            ref_mv.as_mv.col = (short)rvec[k];
            ref_mv.as_mv.row = (short)rvec[rows * cols + k];
            o[5] = (int)vp8_variance16x16_c(src_base + b.src, stride, ref_base + bd.pre + best.as_mv.row * stride + best.as_mv.col, stride, &sse0);
            o[2] = step(x, &b, &bd, &best, &ref_mv, cost ? error_per_bit : 0, &fn, mvcost, &distortion, &sse);
            o[0] = best.as_mv.col;
            o[1] = best.as_mv.row;
            o[3] = distortion;
            o[4] = (int)sse;
        }
    free(x);
    return 0;
}
