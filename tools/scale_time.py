"""Dev aid (GPU): vp8hip_frames_scale_async on a batch of kf_1920x1080 frames left as tiles by one launch, then the same calls from
the raster form.  Device events around each call; GB/s by the plan's byte model (the source rows each plane's path reads, at the
plane's picture width, plus the destination bytes).
   python3 tools/scale_time.py [frames (8192)] [timed calls (20)] [--check]"""
import os
import sys

import torch  # first: the library then shares torch's HIP runtime

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import numpy as np  # noqa: E402

import scale_reference as S  # noqa: E402
from vp8_testlib import ivf_path, load_package  # noqa: E402

CALLS = ((960, 540, 1), (224, 224, 1), (1440, 810, 1), (1920, 1080, 1))


def rows_read(sw, sh, dw, dh, filt):
    """distinct source rows a plane's path reads"""
    path, f = S.plane_path(sw, sh, dw, dh, filt)
    y = np.arange(dh)
    if path == S.COPY:
        return sh
    if path in (S.DOWN2, S.DOWN4, S.DOWN8, S.DOWN34, S.DOWN38):
        if not f:
            return dh
        return min(sh, {S.DOWN2: 2 * dh, S.DOWN4: 4 * dh, S.DOWN8: 8 * dh, S.DOWN34: 4 * dh // 3, S.DOWN38: (8 * dh + 2) // 3}[path])
    if path == S.POINT:
        return len(np.unique(y * sh // dh))
    dy = (sh << 16) // dh
    maxy = ((sh - 1) << 16) - 1
    if path == S.BILIN8:
        yy = np.where(y == 0, 0, np.minimum(y * dy, maxy))
    else:
        y0 = 32768 if dh < sh else (sh << 16) // dh - 32768
        yy = np.maximum(np.where(y == 0, y0, np.minimum(y0 + y * dy, maxy)), 0)
    iy = yy >> 16
    return len(np.unique(np.concatenate([iy, np.minimum(iy + 1, sh - 1)])))


def byte_model(w, h, dw, dh, f):
    c = lambda v: (v + 1) >> 1
    src = rows_read(w, h, dw, dh, f) * w + 2 * rows_read(c(w), c(h), c(dw), c(dh), f) * c(w)
    return src + S.i420_size(dw, dh)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    n = int(args[0]) if args else 8192
    reps = int(args[1]) if len(args) > 1 else 20
    P = load_package()
    os.environ["VP8HIP_RECON"] = "simt"
    name = "kf_1920x1080"
    w, h, frames = P.read_ivf(ivf_path(name))
    ctx = P.Vp8Hip(0)
    ctx.configure(w, h, n, n)
    parser = P.Parser()
    for i, data in enumerate(frames[:n]):
        ctx.sync()
        hdr, _ = ctx.parse_into_slot_compact(parser, data, i)
        parser.swap(hdr)
    parser.close()
    for i in range(len(frames), n):
        ctx.ir_copy(i, i % len(frames))
    ctx.decode([(i, i, None) for i in range(n)], P.STAGE_ALL)
    ctx.sync()
    st = ctx.stats()
    print(f"{name} x {n}: one launch, recon {st.recon_ms:.2f} ms; memory {ctx.memory_usage()}")
    fbs = list(range(n))
    outs = {(dw, dh): torch.empty((n, S.i420_size(dw, dh)), dtype=torch.uint8, device="cuda:0") for dw, dh, _ in CALLS}
    for form in ("tiles", "raster"):
        if form == "raster":
            ctx.frames_to_raster(0, n)
            ctx.sync()
        for dw, dh, f in CALLS:
            out = outs[(dw, dh)]
            for _ in range(3):
                ctx.frames_scaled(fbs, dw, dh, f, out=out)
            torch.cuda.synchronize()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            for _ in range(reps):
                ctx.frames_scaled(fbs, dw, dh, f, out=out)
            ev[1].record()
            torch.cuda.synchronize()
            ms = ev[0].elapsed_time(ev[1]) / reps
            gb = byte_model(w, h, dw, dh, f) * n / 1e9
            print(f"from {form:6s} {dw}x{dh} f{f}: {ms:8.3f} ms per call of {n} frames, {gb:6.2f} GB by the byte model, "
                  f"{gb / ms:6.3f} TB/s, {n * w * h / ms / 1e6:7.1f} Gpix/s of source")
    ctx.close()


if __name__ == "__main__":
    main()
