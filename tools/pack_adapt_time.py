"""Dev aid (GPU): Vp8Hip.frames_pack_adapt (all flags) against Vp8Hip.frames_pack on tools/pack_time.py's jobs: 1920x1080, a batch
(256), qindex 10 and 40, 1 and 8 token partitions.  Per case the bytes a frame of both calls and the ms a call, device events around
each call after a warm-up, in the order A B B A over (frames_pack, frames_pack_adapt), both rounds printed and their spread
reported.  `cap` is what the content needs, as in pack_time.py.  Job 0's inputs and frames can be kept (--dump FILE.npz) and restated
on the CPU afterwards (--restate FILE.npz, no GPU: bytes of the default and of the adapted frame by tests/pack_adapt_reference.py,
compared with the device's).  The kernels' shares come from a run of their own:
   rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 tools/pack_adapt_time.py 256 --profile
(--profile: one call of each kind, a kernel of torch's between them; nothing is timed).
   python3 tools/pack_adapt_time.py [jobs (256)] [timed calls (3)] [--profile] [--dump FILE.npz] [--out FILE]
   python3 tools/pack_adapt_time.py --restate FILE.npz [--out FILE]"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
sys.path.insert(0, HERE)


def option(name):
    if name not in sys.argv:
        return None
    v = sys.argv[sys.argv.index(name) + 1]
    sys.argv.remove(v)
    return v


def restate(path, say):
    import pack_adapt_reference as A
    z = np.load(path)
    for q in (10, 40):
        for lp in (0, 3):
            r = A.restate(z["mv"], z[f"coef_q{q}"], qindex=q, log2_parts=lp)
            dev_plain, dev_adapt = z[f"plain_q{q}_p{lp}"].tobytes(), z[f"adapt_q{q}_p{lp}"].tobytes()
            say(f"qindex {q}, {1 << lp} partition(s), job 0 restated: default tables {len(r['default'])} bytes, adapted {len(r['data'])} bytes "
                f"({100 - 100 * len(r['data']) / len(r['default']):.1f} % fewer); {r['info'][16]} coefficient and {r['info'][17]} vector probabilities "
                f"updated, prob_skip_false {r['info'][18]}, estimated saving {r['info'][19]} bits; the device's frames are "
                f"{'equal' if (dev_plain, dev_adapt) == (r['default'], r['data']) else 'DIFFERENT'}")


def main():
    out_path, dump, restated = option("--out"), option("--dump"), option("--restate")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    if restated:
        restate(restated, say)
    else:
        measure(say, dump)
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


def measure(say, dump):
    import torch  # first: the library then shares torch's HIP runtime
    from rgb_time import timed
    from pack_time import make_jobs
    from vp8_testlib import load_package
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    profile = "--profile" in sys.argv
    n = int(args[0]) if args else 256
    reps = int(args[1]) if len(args) > 1 else 3
    P = load_package()
    ctx, jobs, mv, coef = make_jobs(P, n)
    say(f"kf_1920x1080 x {n} frame buffers, {ctx.g.aligned_h // 16 * (ctx.g.aligned_w // 16)} macroblocks a picture; {reps} timed calls after 1")
    kept = {"mv": mv[0].cpu().numpy()}
    summary = []
    for q in (10, 40):
        ctx.frames_quant(jobs, mv, q, want=(), out_coef=coef)
        kept[f"coef_q{q}"] = coef[0].cpu().numpy()
        _, info = ctx.frames_pack(mv, coef, qindex=q, cap=8 << 20)
        info = info.cpu().numpy()
        assert not (info[:, 0] & 7).any(), info[:, 0]
        cap = (int(info[:, 1].max()) * 5 // 4 + 65535) // 65536 * 65536
        for lp in (0, 3):
            data = torch.empty((n, cap), dtype=torch.uint8, device="cuda:0")
            inf16 = torch.empty((n, 16), dtype=torch.int32, device="cuda:0")
            inf32 = torch.empty((n, 32), dtype=torch.int32, device="cuda:0")
            calls = {"frames_pack": lambda: ctx.frames_pack(mv, coef, qindex=q, cap=cap, log2_parts=lp, out_data=data, out_info=inf16),
                     "frames_pack_adapt": lambda: ctx.frames_pack_adapt(mv, coef, qindex=q, cap=cap, log2_parts=lp, out_data=data, out_info=inf32)}
            tag = f"qindex {q}, {n} jobs, {1 << lp} partition(s)"
            if profile:
                for name, fn in calls.items():
                    torch.cuda.synchronize()
                    torch.full((64,), 1.0, device="cuda:0").sum()      # (a kernel of another name between the calls, to cut the trace at)
                    torch.cuda.synchronize()
                    fn()
                    say(f"profiled call: {name}, {tag}")
                torch.cuda.synchronize()
                continue
            size, frames = {}, {}
            for name, fn in calls.items():
                fn()
                torch.cuda.synchronize()
                i = (inf16 if name == "frames_pack" else inf32).cpu().numpy()
                assert not (i[:, 0] & 7).any(), (name, i[:, 0])
                size[name] = i[:, 1].astype(np.int64)
                frames[name] = data[0, :int(i[0, 1])].cpu().numpy()
                if name == "frames_pack_adapt":
                    say(f"{tag}: frames_pack_adapt updates {i[:, 16].mean():.0f} coefficient and {i[:, 17].mean():.1f} vector probabilities a frame, "
                        f"prob_skip_false {int(i[:, 18].min())} .. {int(i[:, 18].max())}, estimated saving {i[:, 19].mean():.0f} bits a frame")
            kept[f"plain_q{q}_p{lp}"], kept[f"adapt_q{q}_p{lp}"] = frames["frames_pack"], frames["frames_pack_adapt"]
            ms = {name: [] for name in calls}
            for order in (("frames_pack", "frames_pack_adapt"), ("frames_pack_adapt", "frames_pack")):     # A B B A
                for name in order:
                    ms[name].append(timed(calls[name], 1, reps))
                    print(f"{name:20s} {tag}: {ms[name][-1]:10.4f} ms per call", flush=True)
            a, b = (sum(ms[k]) / 2 for k in calls)
            spread = max(abs(v[0] - v[1]) / (sum(v) / 2) for v in ms.values()) * 100
            pa, pb = size["frames_pack"].mean(), size["frames_pack_adapt"].mean()
            summary.append(f"{tag}: frames_pack {pa:9.0f} bytes a frame, {a:9.3f} ms a call; frames_pack_adapt {pb:9.0f} bytes a frame "
                           f"({100 - 100 * pb / pa:4.1f} % fewer), {b:9.3f} ms a call ({100 * b / a - 100:+5.1f} %); spread between the rounds at most "
                           f"{spread:3.1f} %; job 0: {len(frames['frames_pack'])} and {len(frames['frames_pack_adapt'])} bytes")
            del data, inf16, inf32
    ctx.close()
    del os.environ["VP8HIP_RECON"]
    if dump and not profile:
        np.savez_compressed(dump, **kept)
    say("--- means over the two rounds")
    for s in summary:
        say(s)


if __name__ == "__main__":
    main()
