"""Dev aid (GPU): the key-frame packer (Vp8Hip.frames_pack_key) at 1920x1080 (8160 macroblocks a picture) over 1 job and over a
batch (256), at qindex 10 and 40, with 1 and with 8 token partitions.  Modes and levels are frames_intra's own on kf_1920x1080's
decoded key frames (job i: frame buffer i).  Beside it, in the same process and not the code under test: frames_pack on
tools/pack_time.py's jobs (frame buffer i against i + 1) and frames_intra (modes and levels alone) on the same pictures.  The order
inside a round is A B B A over (the call, the yardsticks), two rounds, both printed (--out keeps their means and the spread).
Device events around each call after warm-up.  `cap` is what the content needs (the largest frame of the batch and a quarter
more).  Coder decisions are counted by the restatement (tests/pack_key_reference.py) for job 0, whose bytes are compared too.
The kernels' shares come from a run of their own:
   rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 tools/pack_key_time.py 256 --profile
(--profile: one call of each kind, a kernel of torch's between them; nothing is timed or counted), whose kernel trace
--trace FILE sums by call and kernel (no GPU).
   python3 tools/pack_key_time.py [jobs (256)] [timed calls (3)] [--no-count] [--profile] [--out FILE] | --trace FILE"""
import csv
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
sys.path.insert(0, HERE)


def trace(path):
    """the kernel trace of a --profile run: per profiled call (cut at the kernels that are not the packer's) the ms by kernel"""
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    calls, cur = [], {}
    for r in rows:
        name = r["Kernel_Name"].split("(")[0]
        if not name.startswith("vp8_pack"):
            if cur:
                calls.append(cur)
            cur = {}
            continue
        cur[name] = cur.get(name, 0.0) + (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
    if cur:
        calls.append(cur)
    for i, c in enumerate(calls):
        print(f"call {i:2d}: " + "  ".join(f"{k.replace('vp8_pack_', '').replace('_kernel', '')} {v:9.3f}" for k, v in c.items()))


def main():
    if "--trace" in sys.argv:
        return trace(sys.argv[sys.argv.index("--trace") + 1])
    import torch  # first: the library then shares torch's HIP runtime
    from rgb_time import timed
    from vp8_testlib import load_package
    import pack_key_reference as K
    from pack_time import make_jobs
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    if out_path:
        args.remove(out_path)
    profile = "--profile" in sys.argv
    count = "--no-count" not in sys.argv and not profile
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

    def spread(key):
        return abs(times[key][0] - times[key][1]) / mean(key) * 100

    ctx, jobs, mv, coef = make_jobs(P, n)
    rows, cols = ctx.g.aligned_h // 16, ctx.g.aligned_w // 16
    fbs = list(range(n))
    kcoef = torch.empty_like(coef)
    modes = torch.empty((n, rows, cols, 32), dtype=torch.uint8, device="cuda:0")
    say(f"kf_1920x1080 x {n} frame buffers, {rows * cols} macroblocks a picture; {reps} timed calls after 1; pack_key_bound {ctx.pack_key_bound(0)} / "
        f"{ctx.pack_key_bound(3)} bytes (1 / 8 partitions)")
    summary = []
    for q in (10, 40):
        ctx.frames_intra(fbs, q, want=(), out_coef=kcoef, out_modes=modes)
        ctx.frames_quant(jobs, mv, q, want=(), out_coef=coef)
        _, info = ctx.frames_pack_key(modes, kcoef, qindex=q, cap=16 << 20)
        info = info.cpu().numpy()
        assert not info[:, 0].any(), info[:, 0]
        cap = (int(info[:, 1].max()) * 5 // 4 + 65535) // 65536 * 65536
        _, pinfo = ctx.frames_pack(mv, coef, qindex=q, cap=8 << 20)
        pcap = (int(pinfo[:, 1].max()) * 5 // 4 + 65535) // 65536 * 65536
        say(f"qindex {q}: key frames of {int(info[:, 1].min())} .. {int(info[:, 1].max())} bytes, mean {info[:, 1].mean():.0f}; first partition mean "
            f"{info[:, 2].mean():.0f}; skipped macroblocks mean {info[:, 11].mean():.0f}; B_PRED macroblocks mean {info[:, 12].mean():.0f}; cap {cap}; "
            f"the inter frames of frames_pack on the same pictures: mean {pinfo[:, 1].float().mean():.0f} bytes, first partition mean {pinfo[:, 2].float().mean():.0f}")
        puts = {}
        data, inf = ctx.frames_pack_key(modes[:1], kcoef[:1], qindex=q, cap=cap, log2_parts=3)
        mine = P.pack_frames(data, inf)[0]
        if count:                                            # (the tokens and their contexts do not depend on the partitions: one count)
            want = K.restate(modes[0].cpu().numpy(), kcoef[0].cpu().numpy(), qindex=q, log2_parts=3, count_puts=True, display=(ctx.width, ctx.height))
            assert mine == want["data"], "job 0 differs from the restatement"
            puts = {3: want["puts"], 0: [want["puts"][0], sum(want["puts"][1:])]}
            say(f"qindex {q}, 8 partitions, job 0: {len(mine)} bytes equal the restatement's; decisions: first partition {puts[3][0]} (1094 of them "
                f"the header's), token partitions {puts[3][1:]} (sum {puts[0][1]})")
        if profile:
            for m in (n, 1):
                for lp in (0, 3):
                    torch.cuda.synchronize()
                    torch.full((64,), 1.0, device="cuda:0").sum()      # (a kernel of another name between the calls, to cut the trace at)
                    torch.cuda.synchronize()
                    ctx.frames_pack_key(modes[:m], kcoef[:m], qindex=q, cap=cap, log2_parts=lp)
                    say(f"profiled call: qindex {q}, {m} jobs, {1 << lp} partition(s)")
            torch.cuda.synchronize()
            continue
        for m in (1, n):
            data = torch.empty((m, cap), dtype=torch.uint8, device="cuda:0")
            pdata = torch.empty((m, pcap), dtype=torch.uint8, device="cuda:0")
            inf = torch.empty((m, 16), dtype=torch.int32, device="cuda:0")
            spare_c, spare_m = kcoef[:m].clone(), modes[:m].clone()         # (frames_intra's own output beside what the packer reads)
            tag = f"qindex {q}, {m} job{'s' if m > 1 else ''}"

            def ours(rd):
                for lp in (0, 3):
                    row(("key", q, m, lp), f"frames_pack_key, {1 << lp} partition(s)                     {tag}, round {rd}",
                        lambda: ctx.frames_pack_key(modes[:m], kcoef[:m], qindex=q, cap=cap, log2_parts=lp, out_data=data, out_info=inf))

            def yardsticks(rd):
                for lp in (0, 3):
                    row(("pack", q, m, lp), f"yardstick  frames_pack, {1 << lp} partition(s)                {tag}, round {rd}",
                        lambda: ctx.frames_pack(mv[:m], coef[:m], qindex=q, cap=pcap, log2_parts=lp, out_data=pdata, out_info=inf))
                row(("intra", q, m), f"yardstick  frames_intra, modes and levels alone             {tag}, round {rd}",
                    lambda: ctx.frames_intra(fbs[:m], q, want=(), out_coef=spare_c, out_modes=spare_m))
            for rd in range(2):                              # A B B A
                (ours if rd == 0 else yardsticks)(rd)
                (yardsticks if rd == 0 else ours)(rd)
            for lp in (0, 3):
                t, tp, ti = mean(("key", q, m, lp)), mean(("pack", q, m, lp)), mean(("intra", q, m))
                line = (f"{tag}, {1 << lp} partition(s): frames_pack_key {t:10.4f} ms a call (spread {spread(('key', q, m, lp)):4.1f} %), {t / m:9.4f} ms a "
                        f"frame; frames_pack {tp:10.4f} ms (spread {spread(('pack', q, m, lp)):4.1f} %): the key packer is {t / tp:6.2f} times that; "
                        f"frames_intra {ti:9.4f} ms: {t / ti:6.2f} times that")
                if m == 1 and count:
                    line += f"; slowest token lane {max(puts[lp][1:])} decisions, first partition {puts[lp][0]} decisions"
                summary.append(line)
            del data, pdata, inf, spare_c, spare_m
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
