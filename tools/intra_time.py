"""Dev aid (GPU): intra modes and levels of key-frame macroblocks at 1920x1080 (8160 macroblocks a picture, 254 wavefront steps) over
1 job and over a batch (256): qindex 10 and 40, with and without the B_PRED chain, bmode_last 3 and 9, every output and levels
alone, and, in the same process over the same frame buffers, frames_quant with every output (job i against job i + 1, no vectors):
the same transforms and quantiser without the wavefront.  The pictures are kf_1920x1080's decoded key frames in raster form.  The
order inside a round is A B B A over (frames_intra, frames_quant), two rounds, both printed (--out keeps their means and the spread
between them).  Device events around each call after warm-up.
   python3 tools/intra_time.py [jobs (256)] [timed calls (3)] [--out FILE]"""
import os
import sys

import torch  # first: the library then shares torch's HIP runtime

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
sys.path.insert(0, HERE)
from rgb_time import timed  # noqa: E402
from vp8_testlib import ivf_path, load_package  # noqa: E402


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    if out_path:
        args.remove(out_path)
    n = int(args[0]) if args else 256
    reps = int(args[1]) if len(args) > 1 else 3
    P = load_package()
    lines, times = [], {}

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def row(key, what, fn):
        ms = timed(fn, 1, reps)
        times.setdefault(key, []).append(ms)
        print(f"{what:100s} {ms:10.4f} ms per call", flush=True)

    def mean(key):
        return sum(times[key]) / len(times[key])

    w, h, frames = P.read_ivf(ivf_path("kf_1920x1080"))
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
    ctx.frames_to_raster(0, n)
    ctx.sync()
    rows, cols = ctx.g.aligned_h // 16, ctx.g.aligned_w // 16
    steps = cols + 2 * (rows - 1)
    say(f"kf_1920x1080 x {n} frame buffers (raster), {rows * cols} macroblocks a picture, {steps} wavefront steps; {reps} timed calls after 1")
    iplanes, qplanes = tuple(P.INTRA_PLANES), tuple(P.QUANT_PLANES)
    rsize = P.intra_sizes(w, h)[3]
    for m in (1, n):
        fbs = list(range(m))
        pairs = [(i, (i + 1) % n) for i in range(m)]
        coef = torch.empty((m, rows, cols, 25, 16), dtype=torch.int16, device="cuda:0")
        eob = torch.empty((m, rows, cols, 32), dtype=torch.uint8, device="cuda:0")
        modes = torch.empty((m, rows, cols, 32), dtype=torch.uint8, device="cuda:0")
        st5 = torch.empty((m, 5, rows, cols), dtype=torch.int32, device="cuda:0")
        rec = torch.empty((m, rsize), dtype=torch.uint8, device="cuda:0")
        every = dict(want=(), out_coef=coef, out_eob=eob, out_stats=st5, out_rec=rec, out_modes=modes)

        def ours(rd):
            tag = f"{m} job{'s' if m > 1 else ''}, round {rd}"
            for q in (10, 40):
                for last in (3, 9):
                    row(("all", q, last, m), f"frames_intra q {q:3d}, bmode_last {last}, every output          {tag}",
                        lambda: ctx.frames_intra(fbs, q, bmode_last=last, planes=iplanes, **every))
                    row(("levels", q, last, m), f"frames_intra q {q:3d}, bmode_last {last}, levels alone          {tag}",
                        lambda: ctx.frames_intra(fbs, q, bmode_last=last, want=(), out_coef=coef))
                row(("all", q, "none", m), f"frames_intra q {q:3d}, no B_PRED, every output             {tag}",
                    lambda: ctx.frames_intra(fbs, q, bpred=False, planes=iplanes, **every))
                row(("levels", q, "none", m), f"frames_intra q {q:3d}, no B_PRED, levels alone             {tag}",
                    lambda: ctx.frames_intra(fbs, q, bpred=False, want=(), out_coef=coef))

        def yardstick(rd):
            tag = f"{m} job{'s' if m > 1 else ''}, round {rd}"
            for q in (10, 40):
                row(("quant", q, m), f"yardstick  frames_quant q {q:3d}, every output, no vectors   {tag}",
                    lambda: ctx.frames_quant(pairs, None, q, planes=qplanes, want=(), out_coef=coef, out_eob=eob, out_stats=st5, out_rec=rec))
        for rd in range(2):                              # A B B A
            (ours if rd == 0 else yardstick)(rd)
            (yardstick if rd == 0 else ours)(rd)
        if m == 1:
            share = ctx.frames_intra(fbs, 40, want=("modes",))["modes"][0, :, :, 0]
            say(f"   q 40, bmode_last 3, frame buffer 0: B_PRED macroblocks {int((share == 4).sum())} of {rows * cols}")
        del coef, eob, modes, st5, rec
        torch.cuda.empty_cache()
    ctx.close()
    for m in (1, n):
        say(f"--- {m} job{'s' if m > 1 else ''}: means over the two rounds, ms a call (spread between the rounds in % of the mean)")
        for q in (10, 40):
            for last in (3, 9, "none"):
                a, lv = mean(("all", q, last, m)), mean(("levels", q, last, m))
                t = times[("all", q, last, m)]
                say(f"q {q:3d} bmode_last {str(last):4s}: every output {a:10.4f} ({abs(t[0] - t[1]) / a * 100:4.1f} %)  levels alone {lv:10.4f}  "
                    f"a wavefront step {a / steps * 1e3:8.2f} us  a macroblock of a job {a / (rows * cols) * 1e3:7.3f} us  pictures a second "
                    f"{m / a * 1e3:9.1f} | frames_quant every output {mean(('quant', q, m)):9.4f}: intra / it {a / mean(('quant', q, m)):8.1f}")
    for q in (10, 40):
        say(f"q {q:3d}: {n} jobs / 1 job, every output: bmode_last 3 {mean(('all', q, 3, n)) / mean(('all', q, 3, 1)):6.2f}, 9 "
            f"{mean(('all', q, 9, n)) / mean(('all', q, 9, 1)):6.2f}, no B_PRED {mean(('all', q, 'none', n)) / mean(('all', q, 'none', 1)):6.2f}")
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
