/* Driver of tests/golden/make_motion_fixtures.py: calls the REFERENCE's vp8_full_search_sad_c (vp8/encoder/mcomp.c), vp8_sad16x16_c
 * and vp8_variance16x16_c, as oracle/_ref/libvpxref.so exports them, for every macroblock of a picture pair.  It fills the few fields
 * of MACROBLOCK / BLOCK / BLOCKD / vp8_variance_fn_ptr_t the search reads, sets the UMV bounds as vp8/encoder/encodeframe.c sets
 * them, and records what came back.  The pictures arrive bordered by 32 replicated pixels (the reference's border extension), made
 * by the caller.  Built into a scratch directory by make_motion_fixtures.py; nothing of it is loaded by the tests. */
#include <limits.h>
#include <stdlib.h>
#include <string.h>

#include "vpx_config.h"
#include "vpx_rtcd.h"
#include "vp8/encoder/block.h"
#include "vp8/encoder/variance.h"

#define BORDER 32              /* VP8BORDERINPIXELS */
#define RESULTS 7              /* per macroblock: col, row (whole pixels), plain SAD at the best vector, SAD at (0, 0), SSE, VAR, SRCVAR */

static int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

/* src / ref: pictures of (w + 64) x (h + 64) bytes, the coded area at (32, 32).  centre: NULL or int32 [2][rows][cols] (x, y).  cost:
 * NULL or int32 [2][2 d + 1].  out: int32 [rows * cols][RESULTS].  Returns 0. */
int motion_ref_run(const unsigned char *src, const unsigned char *ref, int w, int h, int d, const int *centre, const int *cost, int sad_per_bit,
                   int *out)
{
    const int stride = w + 2 * BORDER, cols = w / 16, rows = h / 16;
    MACROBLOCK *x = calloc(1, sizeof *x);
    BLOCK b;
    BLOCKD bd;
    vp8_variance_fn_ptr_t fn;
    static int zeros[2][4096 + 1];
    static int sadcost[2][256];
    static unsigned char offs[16];
    int *mvcost[2] = {zeros[0] + 2048, zeros[1] + 2048};
    unsigned char *src_base = (unsigned char *)src + BORDER * stride + BORDER, *ref_base = (unsigned char *)ref + BORDER * stride + BORDER;

    memset(&b, 0, sizeof b);
    memset(&bd, 0, sizeof bd);
    memset(&fn, 0, sizeof fn);
    memset(sadcost, 0, sizeof sadcost);
    memset(offs, 128, sizeof offs);
    fn.sdf = vp8_sad16x16_c;
    fn.vf = vp8_variance16x16_c;
    if (cost)
        for (int k = 0; k < 2; k++)
            for (int i = 0; i <= 2 * d; i++) sadcost[k][i] = cost[k * (2 * d + 1) + i];
    x->mvsadcost[0] = sadcost[0] + d;
    x->mvsadcost[1] = sadcost[1] + d;
    x->errorperbit = 1;
    for (int my = 0; my < rows; my++)
        for (int mx = 0; mx < cols; mx++) {
            int *o = out + (my * cols + mx) * RESULTS;
            int_mv ref_mv, centre_mv;
            unsigned int sse = 0;
            x->mv_row_min = -((my * 16) + (BORDER - 16));
            x->mv_row_max = ((rows - 1 - my) * 16) + (BORDER - 16);
            x->mv_col_min = -((mx * 16) + (BORDER - 16));
            x->mv_col_max = ((cols - 1 - mx) * 16) + (BORDER - 16);
            b.base_src = &src_base;
            b.src = my * 16 * stride + mx * 16;
            b.src_stride = stride;
            bd.base_pre = &ref_base;
            bd.pre = my * 16 * stride + mx * 16;
            bd.pre_stride = stride;
            ref_mv.as_mv.col = (short)clampi(centre ? centre[my * cols + mx] : 0, x->mv_col_min, x->mv_col_max);
            ref_mv.as_mv.row = (short)clampi(centre ? centre[rows * cols + my * cols + mx] : 0, x->mv_row_min, x->mv_row_max);
            centre_mv.as_mv.col = ref_mv.as_mv.col << 3;
            centre_mv.as_mv.row = ref_mv.as_mv.row << 3;
            const int var = vp8_full_search_sad_c(x, &b, &bd, &ref_mv, sad_per_bit, d, &fn, mvcost, &centre_mv);
            const unsigned char *what = src_base + b.src, *in_what = ref_base + bd.pre;
            const unsigned char *best = in_what + bd.bmi.mv.as_mv.row * stride + bd.bmi.mv.as_mv.col;
            o[0] = bd.bmi.mv.as_mv.col;
            o[1] = bd.bmi.mv.as_mv.row;
            o[2] = (int)vp8_sad16x16_c(what, stride, best, stride, INT_MAX);
            o[3] = (int)vp8_sad16x16_c(what, stride, in_what, stride, INT_MAX);
            o[5] = (int)vp8_variance16x16_c(what, stride, best, stride, &sse);
            o[4] = (int)sse;
            if (o[5] != var) return 1;                 /* (the search returns the variance at its result: all mv costs are 0) */
            o[6] = (int)vp8_variance16x16_c(what, stride, offs, 0, &sse);
        }
    free(x);
    return 0;
}
