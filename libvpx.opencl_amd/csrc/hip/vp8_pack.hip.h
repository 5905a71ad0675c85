// Internal to libvp8hip.so: what the plan of vp8hip_frames_pack_async (vp8hip_pack.hip) and its kernels (vp8_pack.hip) share -- the
// launch's arguments, the layout of the scratch, the bounds the regions and vp8hip_pack_bound are made of, and the probability
// tables, taken from host/vp8_tables.c by inclusion (a translation unit's own copy with internal linkage; clang makes a constant
// array that device code reads a device constant too).
#pragma once
#include <stdint.h>
#include <stddef.h>

#define VP8_TABLES_H                    // (vp8_tables.c's own header declares the arrays extern: not here)
namespace pack_tables {
#include "../host/vp8_tables.c"
}

#define PACK_MAX_JOBS 1024              // jobs of a launch group (head_of travels in the arguments)
#define PACK_MAX_HEADS 8                // distinct qindex values of a launch group
#define PACK_HEAD_BYTES 64              // VP8HIP_PACK_HEAD_MAX
#define PACK_RECORD_BYTES 32            // a macroblock's plan record
#define PACK_CTR_DWORDS 16              // a job's counters in the scratch
// A put moves the coder by at most 7 bits: range is 128..255 before it and at least 1 after it, so at most 7 renormalisation shifts.
// First partition, per macroblock: skip, inter, two reference puts, four mode puts, and two vector components of at most 12 puts each
// (long form: the flag, ten magnitude bits, the sign): 32 puts, 224 bits.  Tokens, per coefficient: at most 7 tree puts, 11 extra
// bits, the sign: 19 puts; a block is at most 16 of them and an end-of-block put: 305 puts; 25 blocks: 7625 puts, 53375 bits.
#define PACK_MB_FIRST_BYTES 28
#define PACK_MB_TOKEN_BYTES 6672
#define PACK_FLUSH_BYTES 4              // BoolEncoder.finish
#define PACK_FIRST_LIMIT (1u << 19)     // the frame tag has 19 bits for the first partition's size
// A key frame (vp8hip_frames_pack_key_async; vp8_pack_key.hip has its record): ten bytes before the first partition -- the tag, the
// start code, width and height.  First partition, per macroblock: the skip flag, the B_PRED bit of vp8_kf_ymode_tree, sixteen
// sub-block modes at the longest path of vp8_bmode_tree, seven puts, and three puts for the uv mode: 117 puts, 819 bits (a 16x16
// mode is seven puts in all).  The tokens are at most the inter frame's: 24 blocks from step 0, or 25 with sixteen of them from step 1.
#define PACK_KEY_HEADER_BYTES 10
#define PACK_KEY_MB_FIRST_BYTES 103

#define PACK_OVERFLOW 1u
#define PACK_BAD_VECTOR 2u
#define PACK_BAD_LEVEL 4u
#define PACK_CLAMPS 8u
#define PACK_BAD_MODE 16u               // (key frames)
#define PACK_MAX_LEVEL 2114             // DCT_CAT6: 67 + 2047

// a job's counters: [0] status, [1] skipped macroblocks, [2..5] ZEROMV / NEARESTMV / NEARMV / NEWMV, [6] first partition bytes,
// [7..14] token partition bytes
#define PACK_CTR_STATUS 0
#define PACK_CTR_SKIPPED 1
#define PACK_CTR_MODES 2
#define PACK_CTR_FIRST 6
#define PACK_CTR_PARTS 7

// the coder's state where the frame header ends (vp8hip_pack_head of include/vp8hip.h, field for field)
struct PackHead {
    uint32_t bottom, range, bit_count, nbytes;
    int32_t cache;                      // the last byte of `bytes` that is not 0xFF ...
    uint32_t pending, settled, reserved;    // ... the 0xFF bytes behind it, and how many bytes lie before it: settled + 1 + pending = nbytes
    uint8_t bytes[PACK_HEAD_BYTES];
};

// The scratch of a launch group of m jobs: m * PACK_CTR_DWORDS counters, then per job `job_bytes`: the records (PACK_RECORD_BYTES *
// macroblocks), the first partition's region (first_cap bytes), the 1 << log2_parts token regions (part_cap bytes each); every
// piece a multiple of 16.
struct PackLaunch {
    int mb_cols, mb_rows, log2_parts, has_mv;
    int ref_frame, prob_skip, prob_intra, prob_last, prob_gf, version, show_frame;
    uint32_t cap, first_cap, part_cap;
    size_t jobs_off, job_bytes;
    PackHead heads[PACK_MAX_HEADS];
    uint8_t head_of[PACK_MAX_JOBS];
};

// what the kernels of vp8hip_frames_pack_key_async take beside PackLaunch (of which has_mv, ref_frame and the three reference
// probabilities are not read; counter [2] counts the B_PRED macroblocks)
struct PackKey {
    const uint8_t *modes;
    size_t modes_stride;
    int width, height;                  // the display size, 14 bits each in the frame
};

// vp8hip_frames_pack_adapt_async adds, behind the last job's area (adapt_off, a multiple of 256), PACK_ADAPT_JOB_BYTES a job:
//   PACK_ADAPT_COUNTS  1216 uint32: the token counts [4][8][3][12], then per vector component (row, column) 32 branch counts:
//                      is_short_ct[2], sign_ct[2], short_ct[8], bit_ct[10][2] (the count kernel adds to them; zeroed before it)
//   PACK_ADAPT_EFF     the effective probability set, vp8hip_pack_probs' 1104 bytes
//   PACK_ADAPT_FLAG    1104 bytes: 1 where the frame codes an update of that probability
//   PACK_ADAPT_ROWS    the effective coefficient table as the token coder's LDS holds it: 96 rows of 12 bytes
//   PACK_ADAPT_HDR     8 uint32: info[16..19], then prob_intra, prob_last, prob_gf as coded ([2] is prob_skip_false)
// and, at info_off, the 16 uint32 a job that the assemble kernel writes (the call's info has 32).
#define PACK_PROBS_BYTES 1104           // sizeof(vp8hip_pack_probs)
#define PACK_ADAPT_COUNT_DWORDS 1216
#define PACK_ADAPT_COUNTS 0
#define PACK_ADAPT_EFF 4864
#define PACK_ADAPT_FLAG (PACK_ADAPT_EFF + PACK_PROBS_BYTES)
#define PACK_ADAPT_ROWS (PACK_ADAPT_FLAG + PACK_PROBS_BYTES)
#define PACK_ADAPT_HDR (PACK_ADAPT_ROWS + 1152)
#define PACK_ADAPT_JOB_BYTES (PACK_ADAPT_HDR + 32)
#define PACK_ADAPT_HDR_SKIP 2
#define PACK_ADAPT_HDR_INTRA 4
#define PACK_ADAPT_HDR_LAST 5
#define PACK_ADAPT_HDR_GF 6
// The update section behind the host's header prefix: 1056 flags with 8 literal bits each, 35 literal bits (mb_no_coeff_skip, the
// four header probabilities, the two intra update flags), 38 flags with 7 literal bits each: 9843 puts of at most 7 bits, 8613
// bytes, rounded up to a multiple of 16
#define PACK_ADAPT_UPDATE_BYTES 8624

#define PACK_ADAPT_COEF 1
#define PACK_ADAPT_MV 2
#define PACK_ADAPT_SKIP 4
#define PACK_ADAPT_REF 8

struct PackAdapt {
    size_t adapt_off, info_off;
    const uint8_t *probs_in;            // NULL: the defaults
    size_t probs_in_stride;
    uint32_t *info, *counts;            // the call's (32 and 1216 uint32 a job); counts may be NULL
    uint8_t *probs_out;                 // 1104 bytes a job, or NULL
    int flags;
};

// The record of a macroblock, eight dwords: [0] bits 0..24 "block b has a coded level" (b as in frames_quant's coef: Y 0..15, U, V,
// Y2 24; none set: the macroblock is skipped), bits 25..26 the mode (0 ZEROMV, 1 NEARESTMV, 2 NEARMV, 3 NEWMV); [1..5] the blocks'
// ends -- 1 + the last coded zigzag step, 0 for none --, five bits each, six to a dword; [6] the four mode probabilities the
// neighbours give (vp8_mode_contexts[cnt[i]][i]), a byte each; [7] the coded vector difference, row in the low half, int16 each.
#define PACK_NZ_MASK 0x1ffffffu
