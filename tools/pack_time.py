"""Dev aid (GPU): the frame packer (Vp8Hip.frames_pack) at 1920x1080 (8160 macroblocks a picture) over 1 job and over a batch (256),
at qindex 10 and 40, with 1 and with 8 token partitions.  Levels and vectors are frames_motion's / frames_subpel's / frames_quant's
on kf_1920x1080's decoded key frames (job i: frame buffer i against i + 1).  Beside it, in the same process and not the code
under test: frames_quant (levels alone) over the same jobs.  The order inside a round is A B B A over (the call, the yardstick), two
rounds, both printed (--out keeps their means and the spread).  Device events around each call after warm-up.  `cap` is what the
content needs (the largest frame of the batch and a quarter more): the default, vp8hip_pack_bound, is 54 MB a frame here.
Coder decisions are counted by the restatement (tests/pack_reference.py) for job 0, whose bytes are compared too; a lane's
ns per decision is the one-job call over the decisions of its slowest lane.  The kernels' shares come from a run of their own:
   rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 tools/pack_time.py 256 --profile
(--profile: one call of each kind, a kernel of torch's between them; nothing is timed or counted).
   python3 tools/pack_time.py [jobs (256)] [timed calls (5)] [--no-count] [--profile] [--out FILE]"""
import os
import sys

import torch  # first: the library then shares torch's HIP runtime

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
sys.path.insert(0, HERE)
from rgb_time import timed  # noqa: E402
from vp8_testlib import ivf_path, load_package  # noqa: E402
import pack_reference as R  # noqa: E402


def make_jobs(P, n):
    """-> (ctx, jobs, mv, coef): n decoded frame buffers of kf_1920x1080, job i frame buffer i against i + 1, frames_subpel's vectors
    of them and an empty levels tensor for frames_quant (tools/pack_adapt_time.py measures on the same jobs)"""
    os.environ["VP8HIP_RECON"] = "simt"                 # the large launch's kernels: frames left as tiles
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
    ctx.sync()
    rows, cols = ctx.g.aligned_h // 16, ctx.g.aligned_w // 16
    jobs = [(i, (i + 1) % n) for i in range(n)]
    whole = torch.empty((n, 2, rows, cols), dtype=torch.int16, device="cuda:0")
    mv = torch.empty((n, 2, rows, cols), dtype=torch.int16, device="cuda:0")
    coef = torch.empty((n, rows, cols, 25, 16), dtype=torch.int16, device="cuda:0")
    ctx.frames_motion(jobs, 16, planes=(), out_mv=whole)
    ctx.frames_subpel(jobs, start=whole, planes=(), out_mv=mv)
    return ctx, jobs, mv, coef


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    if out_path:
        args.remove(out_path)
    profile = "--profile" in sys.argv                    # one call of each kind and no timing: for a kernel trace
    count = "--no-count" not in sys.argv and not profile
    n = int(args[0]) if args else 256
    reps = int(args[1]) if len(args) > 1 else 5
    P = load_package()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    times = {}

    def row(key, what, fn):
        ms = timed(fn, 1, reps)
        times.setdefault(key, []).append(ms)
        print(f"{what:100s} {ms:10.4f} ms per call", flush=True)
        return ms

    def mean(key):
        return sum(times[key]) / len(times[key])

    ctx, jobs, mv, coef = make_jobs(P, n)
    rows, cols = ctx.g.aligned_h // 16, ctx.g.aligned_w // 16
    say(f"kf_1920x1080 x {n} frame buffers, {rows * cols} macroblocks a picture; {reps} timed calls after 1; pack_bound {ctx.pack_bound(0)} / "
        f"{ctx.pack_bound(3)} bytes (1 / 8 partitions)")
    summary = []
    for q in (10, 40):
        ctx.frames_quant(jobs, mv, q, want=(), out_coef=coef)
        _, info = ctx.frames_pack(mv, coef, qindex=q, cap=8 << 20)
        info = info.cpu().numpy()
        assert not (info[:, 0] & 7).any(), info[:, 0]
        cap = (int(info[:, 1].max()) * 5 // 4 + 65535) // 65536 * 65536
        say(f"qindex {q}: frames of {int(info[:, 1].min())} .. {int(info[:, 1].max())} bytes, mean {info[:, 1].mean():.0f}; first partition mean "
            f"{info[:, 2].mean():.0f}; skipped macroblocks mean {info[:, 11].mean():.0f}; modes (zero, nearest, near, new) "
            f"{info[:, 12:16].mean(axis=0).round().astype(int).tolist()}; cap {cap}")
        puts = {}
        data, inf = ctx.frames_pack(mv[:1], coef[:1], qindex=q, cap=cap, log2_parts=3)
        mine = P.pack_frames(data, inf)[0]
        if count:                                            # (the tokens and their contexts do not depend on the partitions: one count)
            want = R.restate(mv[0].cpu().numpy(), coef[0].cpu().numpy(), qindex=q, log2_parts=3, count_puts=True)
            assert mine == want["data"], "job 0 differs from the restatement"
            puts = {3: want["puts"], 0: [want["puts"][0], sum(want["puts"][1:])]}
            say(f"qindex {q}, 8 partitions, job 0: {len(mine)} bytes equal the restatement's; decisions: first partition {puts[3][0]}, "
                f"token partitions {puts[3][1:]} (sum {puts[0][1]})")
        if profile:
            for m in (n, 1):
                for lp in (0, 3):
                    torch.cuda.synchronize()
                    torch.full((64,), 1.0, device="cuda:0").sum()      # (a kernel of another name between the calls, to cut the trace at)
                    torch.cuda.synchronize()
                    ctx.frames_pack(mv[:m], coef[:m], qindex=q, cap=cap, log2_parts=lp)
                    say(f"profiled call: qindex {q}, {m} jobs, {1 << lp} partition(s)")
            torch.cuda.synchronize()
            continue
        for m in (1, n):
            data = torch.empty((m, cap), dtype=torch.uint8, device="cuda:0")
            inf = torch.empty((m, 16), dtype=torch.int32, device="cuda:0")
            one = coef[:m].clone() if m < n else None       # (frames_quant's own output beside the levels the packer reads)
            tag = f"qindex {q}, {m} job{'s' if m > 1 else ''}"

            def ours(rd):
                for lp in (0, 3):
                    row(("pack", q, m, lp), f"frames_pack, {1 << lp} partition(s)                         {tag}, round {rd}",
                        lambda: ctx.frames_pack(mv[:m], coef[:m], qindex=q, cap=cap, log2_parts=lp, out_data=data, out_info=inf))

            def yardstick(rd):
                out = one if one is not None else coef
                row(("quant", q, m), f"yardstick  frames_quant regular, levels alone              {tag}, round {rd}",
                    lambda: ctx.frames_quant(jobs[:m], mv[:m], q, want=(), out_coef=out))
            for rd in range(2):                              # A B B A
                (ours if rd == 0 else yardstick)(rd)
                (yardstick if rd == 0 else ours)(rd)
            for lp in (0, 3):
                t = mean(("pack", q, m, lp))
                line = (f"{tag}, {1 << lp} partition(s): frames_pack {t:10.4f} ms a call (spread "
                        f"{abs(times[('pack', q, m, lp)][0] - times[('pack', q, m, lp)][1]) / t * 100:4.1f} %), {t / m:9.4f} ms a frame; frames_quant "
                        f"{mean(('quant', q, m)):9.4f} ms a call: the packer is {t / mean(('quant', q, m)):7.1f} times that")
                if m == 1 and count:
                    slow = max(puts[lp][1:])
                    line += (f"; slowest token lane {slow} decisions: at most {t * 1e6 / slow:6.1f} ns a decision and lane; first partition "
                             f"{puts[lp][0]} decisions")
                summary.append(line)
            del data, inf, one
    ctx.close()
    del os.environ["VP8HIP_RECON"]
    say("--- means over the two rounds")
    for s in summary:
        say(s)
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
