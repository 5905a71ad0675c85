/* Driver of tests/golden/make_pack_adapt_fixtures.py: asks the REFERENCE's exported functions (oracle/_ref/libvpxref.so) what they
 * make of count sets -- vp8_tree_probs_from_distribution over vp8_coef_tree, vp8_estimate_entropy_savings on a zeroed VP8_COMP (a
 * key frame without error resilience: default_coef_context_savings over coef_counts alone; it leaves frame_coef_probs and
 * frame_branch_ct), vp8_write_mvprobs on a zeroed VP8_COMP with a bool coder started on a buffer -- and hands out vp8_prob_cost.
 * vp8_coef_encodings and vp8_small_mvencodings are filled with vp8_tokens_from_tree, as the reference's own initialisation does.
 * Built into a scratch directory by make_pack_adapt_fixtures.py; nothing of it is loaded by the tests. */
#include <stdlib.h>
#include <string.h>

#include "vpx_config.h"
#include "vpx_rtcd.h"
#include "vp8/encoder/onyx_int.h"
#include "vp8/common/entropymv.h"
#include "vp8/common/entropymode.h"

int vp8_estimate_entropy_savings(VP8_COMP *cpi);
void vp8_write_mvprobs(VP8_COMP *cpi);

static void trees(void)
{
    static int done;

    if (done) return;
    vp8_tokens_from_tree(vp8_coef_encodings, vp8_coef_tree);
    vp8_tokens_from_tree(vp8_small_mvencodings, vp8_small_mvtree);
    done = 1;
}

void adapt_ref_cost(unsigned *out)
{
    for (int i = 0; i < 256; i++) out[i] = vp8_prob_cost[i];
}

/* counts[12] -> probs[11], branch[11][2] */
void adapt_ref_tree(const unsigned *counts, unsigned char *probs, unsigned *branch)
{
    trees();
    vp8_tree_probs_from_distribution(MAX_ENTROPY_TOKENS, vp8_coef_encodings, vp8_coef_tree, probs, (unsigned int(*)[2])branch, counts, 256, 1);
}

/* counts[1152], base[1056] -> newp[1056], branch[1056][2]; returns the reference's estimate of the saving */
int adapt_ref_savings(const unsigned *counts, const unsigned char *base, unsigned char *newp, unsigned *branch)
{
    VP8_COMP *cpi = calloc(1, sizeof *cpi);
    int s;

    if (!cpi) return -1;
    trees();
    memcpy(cpi->coef_counts, counts, sizeof cpi->coef_counts);
    memcpy(cpi->common.fc.coef_probs, base, sizeof cpi->common.fc.coef_probs);
    s = vp8_estimate_entropy_savings(cpi);
    memcpy(newp, cpi->frame_coef_probs, sizeof cpi->frame_coef_probs);
    memcpy(branch, cpi->frame_branch_ct, sizeof cpi->frame_branch_ct);
    free(cpi);
    return s;
}

/* events[2][2047] (row, column; index 1023 + d), mvc[38] the context before and after -> the bytes written, vp8_stop_encode's
 * padding included; returns their number */
int adapt_ref_mvprobs(const unsigned *events, unsigned char *mvc, unsigned char *bytes, int cap)
{
    VP8_COMP *cpi = calloc(1, sizeof *cpi);
    int n;

    if (!cpi) return -1;
    trees();
    memcpy(cpi->MVcount, events, sizeof cpi->MVcount);
    memcpy(cpi->common.fc.mvc, mvc, 38);
    cpi->mb.mvcost[0] = &cpi->mb.mvcosts[0][mv_max + 1];
    cpi->mb.mvcost[1] = &cpi->mb.mvcosts[1][mv_max + 1];
    vp8_start_encode(cpi->bc, bytes, bytes + cap);
    vp8_write_mvprobs(cpi);
    vp8_stop_encode(cpi->bc);
    n = (int)cpi->bc->pos;
    memcpy(mvc, cpi->common.fc.mvc, 38);
    free(cpi);
    return n;
}
