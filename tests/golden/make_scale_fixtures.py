"""Fixtures of the device scaler (vp8hip_frames_scale_async): what the REFERENCE tree's own scaler, libyuv's I420Scale
(third_party/libyuv/source/scale.c:3762), makes of the frames the reference decoder shows.

    python tests/golden/make_scale_fixtures.py <reference root>

Needs oracle/_ref/libvpxref.so (`make -C oracle ref`).  A small C harness of our own (HARNESS below) is written to a temporary
directory and compiled with -DYUV_DISABLE_ASM -- libyuv's C rows, which is what the generic-gnu build of oracle/_ref is; the
x86 SIMD rows round differently -- against the reference's scale.c / cpu_id.c / md5_utils.c and oracle/_ref/libvpxref.so,
the way oracle/Makefile builds ref_md5.  It decodes with the reference's vpx_codec_* (post-processing off), hands every shown
image to I420Scale(planes, strides, d_w, d_h, dst, dst_w, (dst_w+1)/2, (dst_w+1)/2, dst_w, dst_h, filter) and digests the
packed result.

Writes, next to this file:
    <stream>.scale_<W>x<H>_f<F>.md5   one line per shown frame ("<md5>  scale-WxH-NNNN.i420"), F in {0, 1}
(filter 2, kFilterBox, is checked to give the bytes of filter 1 and not written: ScalePlaneDown tests src_height * 2 >
dst_height, true for every downscale, so ScalePlaneBox is unreachable from I420Scale.)
Nothing at test time reads the reference tree: tests/scale_reference.py restates the paths and reproduces these listings.
"""
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REFLIB = os.path.join(ROOT, "oracle", "_ref")

# stream -> destination sizes; together they send every path through luma and through chroma (tests/scale_reference.py: plan)
CASES = {
    "p_1920x1080": ((960, 540), (480, 270), (240, 135), (1440, 810), (720, 405), (224, 224)),
    "kf_1920x1080": ((1920, 1080),),
    "kf_640x360": ((1920, 1080), (240, 135), (800, 200)),
    "p_arf_176x144": ((22, 18), (352, 288)),
    "kf_odd_67x45": ((67, 45), (200, 150), (34, 23)),
    "p_odd_130x98": ((65, 49),),
    "kf_3840x2160": ((1280, 720), (480, 270)),
    "p_split_352x288": ((264, 216),),
}

HARNESS = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#define VPX_CODEC_DISABLE_COMPAT 1
#include "vpx/vpx_decoder.h"
#include "vpx/vp8dx.h"
#include "md5_utils.h"
#include "third_party/libyuv/include/libyuv/scale.h"

static unsigned rd32(const unsigned char *p) { return p[0] | (p[1] << 8) | (p[2] << 16) | ((unsigned)p[3] << 24); }

int main(int argc, char **argv) {
    if (argc != 6) { fprintf(stderr, "usage: scale_md5 in.ivf dst_w dst_h filter out.md5\n"); return 2; }
    int dw = atoi(argv[2]), dh = atoi(argv[3]), filter = atoi(argv[4]);
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 1; }
    fseek(f, 0, SEEK_END); long n = ftell(f); fseek(f, 0, SEEK_SET);
    unsigned char *buf = malloc(n);
    if (fread(buf, 1, n, f) != (size_t)n) return 1;
    fclose(f);
    if (n < 32 || memcmp(buf, "DKIF", 4)) { fprintf(stderr, "not IVF\n"); return 1; }
    FILE *out = fopen(argv[5], "wb");
    int cw = (dw + 1) / 2, ch = (dh + 1) / 2;
    size_t size = (size_t)dw * dh + 2 * (size_t)cw * ch;
    unsigned char *o = malloc(size);
    vpx_codec_ctx_t c;
    if (vpx_codec_dec_init(&c, vpx_codec_vp8_dx(), NULL, 0)) { fprintf(stderr, "init failed\n"); return 1; }
    long pos = 32; int cnt = 0;
    while (pos + 12 <= n) {
        unsigned sz = rd32(buf + pos); pos += 12;
        if (pos + sz > n) break;
        cnt++;
        if (vpx_codec_decode(&c, buf + pos, sz, NULL, 0)) { fprintf(stderr, "decode error frame %d\n", cnt); return 1; }
        pos += sz;
        vpx_codec_iter_t it = NULL; vpx_image_t *img;
        while ((img = vpx_codec_get_frame(&c, &it))) {
            memset(o, 0xa5, size);
            if (I420Scale(img->planes[0], img->stride[0], img->planes[1], img->stride[1], img->planes[2], img->stride[2],
                          img->d_w, img->d_h, o, dw, o + (size_t)dw * dh, cw, o + (size_t)dw * dh + (size_t)cw * ch, cw,
                          dw, dh, (FilterMode)filter)) { fprintf(stderr, "I420Scale failed\n"); return 1; }
            MD5Context m; unsigned char d[16];
            MD5Init(&m);
            MD5Update(&m, o, size);
            MD5Final(d, &m);
            for (int i = 0; i < 16; i++) fprintf(out, "%02x", d[i]);
            fprintf(out, "  scale-%dx%d-%04d.i420\n", dw, dh, cnt);
        }
    }
    vpx_codec_destroy(&c);
    fclose(out);
    free(o); free(buf);
    return 0;
}
"""


def build(ref, tmp):
    src = os.path.join(tmp, "scale_md5.c")
    with open(src, "w") as f:
        f.write(HARNESS)
    exe = os.path.join(tmp, "scale_md5")
    gen = os.path.join(REFLIB, "gen")
    yuv = os.path.join(ref, "third_party", "libyuv", "source")
    subprocess.run(["gcc", "-O2", "-w", "-DYUV_DISABLE_ASM", f"-I{gen}", f"-I{ref}", "-o", exe, src,
                    os.path.join(yuv, "scale.c"), os.path.join(yuv, "cpu_id.c"), os.path.join(ref, "md5_utils.c"),
                    f"-L{REFLIB}", "-lvpxref", "-lm", f"-Wl,-rpath,{REFLIB}"], check=True)
    return exe


def listing(exe, tmp, name, w, h, flt):
    out = os.path.join(tmp, "out.md5")
    subprocess.run([exe, os.path.join(HERE, name + ".ivf"), str(w), str(h), str(flt), out], check=True)
    with open(out) as f:
        return f.read()


def main():
    ref = sys.argv[1]
    if not os.path.exists(os.path.join(REFLIB, "libvpxref.so")):
        sys.exit("oracle/_ref/libvpxref.so is missing: make -C oracle ref")
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(ref, tmp)
        for name, sizes in CASES.items():
            for w, h in sizes:
                got = {flt: listing(exe, tmp, name, w, h, flt) for flt in (0, 1, 2)}
                assert got[2] == got[1], (name, w, h, "kFilterBox differs from kFilterBilinear")
                for flt in (0, 1):
                    with open(os.path.join(HERE, f"{name}.scale_{w}x{h}_f{flt}.md5"), "w") as f:
                        f.write(got[flt])
                print(name, f"{w}x{h}", len(got[1].splitlines()), "frames")


if __name__ == "__main__":
    main()
