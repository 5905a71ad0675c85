// Internal to libvp8hip.so: the bool coder of the frame packer, shared by vp8_pack.hip (vp8hip_frames_pack_async: the default
// tables, the header complete from the host), vp8_pack_adapt.hip (vp8hip_frames_pack_adapt_async: every job its own tables, the
// header's probability section coded on the device) and vp8_pack_key.hip (vp8hip_frames_pack_key_async: key frames).  What the
// kernels of the three files share above the coder is vp8_pack_tokens.hip.h; each file stays a translation unit of its own.
//
// The bool coder is RFC 6386 section 7.3 with the carry deferred: the last byte that is not 0xFF is held back (cache) with the
// count of 0xFF bytes behind it (pending), so a carry never walks back through stored bytes, and settled bytes leave in whole
// dwords.  Every store is checked against the end of the lane's region; a lane whose region is full goes on counting.
#pragma once
#include <hip/hip_runtime.h>
#include "vp8_pack.hip.h"

#define PACK_CODER_THREADS 64
#define PACK_ROW_BYTES 12               // a (type, band, context) row of 11 probabilities in LDS, read as three dwords
#define PACK_TABLE_DWORDS (96 * PACK_ROW_BYTES / 4)     // the 96 rows of a coefficient table
// vp8_pack_adapt.hip defines it __forceinline__: its first-partition kernel has more calls of the coder than the inliner takes by
// itself, and a coder that is not inlined keeps its state in scratch memory
#ifndef PACK_CODER_INLINE
#define PACK_CODER_INLINE
#endif

struct PackCoder {
    uint32_t low, range;
    int count;                          // shifts until the next byte is complete
    int cache;                          // -1: none yet
    uint32_t pending;
    uint32_t pos, acc;                  // bytes that have left; those of them that wait for their dword
    uint8_t *base;
    uint32_t cap;
};

static __device__ __forceinline__ void pack_sink(PackCoder &e, uint32_t byte)
{
    e.acc |= (byte & 0xffu) << (8 * (e.pos & 3));
    e.pos++;
    if (!(e.pos & 3)) {
        if (e.pos <= e.cap) *(uint32_t *)(e.base + e.pos - 4) = e.acc;
        e.acc = 0;
    }
}

// a complete byte, bit 8 the carry into what came before it
static __device__ __forceinline__ void pack_emit(PackCoder &e, uint32_t b)
{
    if (b & 0x100u) {
        pack_sink(e, (uint32_t)e.cache + 1);
        for (; e.pending; e.pending--) pack_sink(e, 0);
        e.cache = (int)(b & 0xffu);
    } else if (b == 0xffu && e.cache >= 0) {
        e.pending++;
    } else {
        if (e.cache >= 0) pack_sink(e, (uint32_t)e.cache);
        for (; e.pending; e.pending--) pack_sink(e, 0xffu);
        e.cache = (int)b;
    }
}

static __device__ __forceinline__ void pack_put(PackCoder &e, int bit, uint32_t prob)
{
    const uint32_t split = 1 + (((e.range - 1) * prob) >> 8);
    if (bit) {
        e.low += split;
        e.range -= split;
    } else {
        e.range = split;
    }
    int s = __clz((int)e.range) - 24;   // range is 1..255: 0..7 shifts bring it back to 128..255
    e.range <<= s;
    if (s >= e.count) {
        const int c = e.count;          // the byte is bits 24 - c .. 31 - c of low, the carry the bit above
        pack_emit(e, e.low >> (24 - c));
        e.low = (e.low & ((1u << (24 - c)) - 1)) << c;
        s -= c;
        e.count = 8;
    }
    e.low <<= s;
    e.count -= s;
}

// BoolEncoder.finish: the rest of the byte in the making and three more; then what was held back.  Returns the partition's bytes.
static __device__ PACK_CODER_INLINE uint32_t pack_finish(PackCoder &e)
{
    const int c = e.count;
    pack_emit(e, e.low >> (24 - c));
    const uint32_t rest = (e.low & ((1u << (24 - c)) - 1)) << c;
    pack_emit(e, (rest >> 16) & 0xffu);
    pack_emit(e, (rest >> 8) & 0xffu);
    pack_emit(e, rest & 0xffu);
    if (e.cache >= 0) pack_sink(e, (uint32_t)e.cache);
    for (; e.pending; e.pending--) pack_sink(e, 0xffu);
    if ((e.pos & 3) && ((e.pos + 3) & ~3u) <= e.cap) *(uint32_t *)(e.base + (e.pos & ~3u)) = e.acc;
    return e.pos;
}

static __device__ __forceinline__ uint32_t *pack_counters(uint8_t *scratch, int job) { return (uint32_t *)scratch + (size_t)job * PACK_CTR_DWORDS; }
static __device__ __forceinline__ uint8_t *pack_job(uint8_t *scratch, const PackLaunch &L, int job) { return scratch + L.jobs_off + L.job_bytes * (size_t)job; }
static __device__ __forceinline__ uint8_t *pack_adapt_job(uint8_t *scratch, const PackAdapt &A, int job) { return scratch + A.adapt_off + (size_t)PACK_ADAPT_JOB_BYTES * job; }

// RFC 6386 section 17: a vector component in quarter pel, |v| <= 1023, p its 19 probabilities
static __device__ PACK_CODER_INLINE void pack_mv_component(PackCoder &e, int v, const uint8_t *p)
{
    const int x = v < 0 ? -v : v;
    if (x < 8) {
        pack_put(e, 0, p[0]);
        pack_put(e, x >> 2, p[2]);
        pack_put(e, (x >> 1) & 1, p[x < 4 ? 3 : 6]);
        pack_put(e, x & 1, p[x < 4 ? (x < 2 ? 4 : 5) : (x < 6 ? 7 : 8)]);
    } else {
        pack_put(e, 1, p[0]);
        for (int i = 0; i < 3; i++) pack_put(e, (x >> i) & 1, p[9 + i]);
        for (int i = 9; i > 3; i--) pack_put(e, (x >> i) & 1, p[9 + i]);
        if (x & 0xfff0) pack_put(e, (x >> 3) & 1, p[9 + 3]);
    }
    if (x) pack_put(e, v < 0, p[1]);
}

#define PACK_P(j) ((p[(j) >> 2] >> (8 * ((j) & 3))) & 0xffu)
