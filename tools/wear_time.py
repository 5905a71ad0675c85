"""Dev aid (GPU): vp8hip_frames_wear_async and vp8hip_trace_wear_async on a batch of IR slots holding p_dense_1920x1080's key frame and
three inter frames, over and over -- and, in the same run, the yardsticks they are held against, which are not the code under test:
frames_trace over the same jobs and references (tools/trace_time.py's setup: every job has references of its own, entries i, i + 1,
i + 2 of the pool's first half, the destinations in the second, so that what a hop gathers comes from HBM as it would for streams in
lock step), and trace_flow at the sizes of the wear tensors (1920x1080 with 4 bytes an output pixel from either; 224x224 floats).
Device events around each call after warm-up; time per destination byte, and TB/s by tools/trace_time.py's byte model.
   python3 tools/wear_time.py [slots (4096, or as many as fit beside the pools)] [timed calls (20)] [--out FILE]"""
import os
import sys

import torch  # first: the library then shares torch's HIP runtime
import numpy as np

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
    reps = int(args[1]) if len(args) > 1 else 20
    P = load_package()
    w, h, frames = P.read_ivf(ivf_path("p_dense_1920x1080"))
    nmb = ((w + 15) // 16) * ((h + 15) // 16)
    entry = P.trace_size(w, h)
    per_frame = nmb * 960 + 4 * entry                   # a slot, and a reference entry and a destination entry of either pool
    free, _ = torch.cuda.mem_get_info(0)
    n = int(args[0]) if args else min(4096, int(free * 0.8) // per_frame)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    ctx = P.Vp8Hip(0)
    ctx.configure(w, h, 1, n)
    parser = P.Parser()
    kinds = []
    for i, data in enumerate(frames[:min(4, n)]):
        ctx.sync()
        hdr, _ = ctx.parse_into_slot_compact(parser, data, i)
        parser.swap(hdr)
        kinds.append("key" if hdr.frame_type == 0 else "inter")
    parser.close()
    for i in range(len(kinds), n):
        ctx.ir_copy(i, i % len(kinds))
    ctx.sync()
    before = ctx.memory_usage()
    say(f"p_dense_1920x1080 ({', '.join(kinds)}) x {n} slots; {reps} timed calls after 3; memory {before}")
    n_inter = sum(kinds[i % len(kinds)] == "inter" for i in range(n))
    src_side = nmb * (128 + 64)
    per_byte = {}

    def row(what, ms, gb, dst):
        say(f"{what:58s} {ms:8.3f} ms per call, {gb:7.2f} GB by the byte model, {gb / ms:6.3f} TB/s, {ms * 1e9 / dst:7.4f} ps per destination byte")
        return ms / dst

    rng = np.random.default_rng(1)
    traces, wear = ctx.trace_pool(2 * n), ctx.wear_pool(2 * n)
    some = torch.from_numpy(np.stack([rng.integers(0, w, (4, h, w)), rng.integers(0, h, (4, h, w))], -1).astype(np.int16)).to("cuda:0")
    some_w = torch.from_numpy(rng.integers(0, 256, (4, h, w, 4)).astype(np.uint8)).to("cuda:0")
    for i in range(n):                                  # the references: positions inside the picture; counters of any value
        traces[i] = some[i % 4]
        wear[i] = some_w[i % 4]
    del some, some_w
    jobs = ctx.job_array([(i, n + i, (i, (i + 1) % n, (i + 2) % n)) for i in range(n)])
    shared = ctx.job_array([(i, n + i, (0, 1, 2)) for i in range(n)])
    keys = ctx.job_array([(i - i % len(kinds), n + i, None) for i in range(n)])
    dst = entry * n
    rounds = 2                                          # the two sides of a comparison alternate: yardstick, call, yardstick, call

    def note(key, v):
        per_byte.setdefault(key, []).append(v)

    def ratio(a, b):
        return sum(per_byte[a]) / sum(per_byte[b])
    for what, arr, gathered in (("references of its own a job", jobs, entry * n_inter), ("three references for all jobs", shared, 0),
                                ("key frames only", keys, None)):
        gb = (dst if gathered is None else src_side * n + gathered + dst) / 1e9
        for _ in range(rounds):
            for name, call, pool in (("yardstick  frames_trace", ctx.frames_trace, traces), ("frames_wear", ctx.frames_wear, wear)):
                ms = timed(lambda: call(arr, pool), 3, reps)
                note((name.split()[-1], what), row(f"{name} {w}x{h}, {what}", ms, gb, dst))
    # control: each call in the other pool's memory (values are data to both), to tell the kernels from where the pools lie
    gb = (src_side * n + entry * n_inter + dst) / 1e9
    for _ in range(rounds):
        ms = timed(lambda: ctx.frames_trace(jobs, wear.view(torch.int16)), 3, reps)
        row("control    frames_trace in the wear pool's memory", ms, gb, dst)
        ms = timed(lambda: ctx.frames_wear(jobs, traces.view(torch.uint8)), 3, reps)
        row("control    frames_wear in the trace pool's memory", ms, gb, dst)
    # (the controls wrote destinations only: the references are as they were)
    ctx.frames_trace(jobs, traces)
    ctx.frames_wear(jobs, wear)

    idx = list(range(n, 2 * n))
    for (gw, gh), fdt, wdt, key in (((w, h), torch.int16, torch.uint8, "display"), ((224, 224), torch.float32, torch.float32, "224")):
        free, _ = torch.cuda.mem_get_info(0)
        m = min(n, int(free * 0.8) // (2 * gh * gw * 4 + 4 * gh * gw * 4))       # (both tensors, as floats)
        size = {} if (gw, gh) == (w, h) else dict(width=gw, height=gh)
        read = min(gw * gh, w * h) * 4 * m              # (a small grid touches a dword per output)
        fout = torch.empty((m, 2, gh, gw), dtype=fdt, device="cuda:0")
        wout = torch.empty((m, 4, gh, gw), dtype=wdt, device="cuda:0")
        for _ in range(rounds):
            ms = timed(lambda: ctx.trace_flow(traces, idx[:m], dtype=fdt, scale=None if fdt == torch.int16 else "pixels", out=fout, **size), 3, reps)
            d = fout[0].numel() * fout.element_size() * m
            note(("flow", key), row(f"yardstick  trace_flow {gw}x{gh} {str(fdt).split('.')[-1]}, 2 planes, {m} entries", ms, (read + d) / 1e9, d))
            ms = timed(lambda: ctx.trace_wear(wear, idx[:m], dtype=wdt, scale=None if wdt == torch.uint8 else 1.0 / 255, out=wout, **size), 3, reps)
            d = wout[0].numel() * wout.element_size() * m
            note(("wear", key), row(f"trace_wear {gw}x{gh} {str(wdt).split('.')[-1]}, 4 planes, {m} entries", ms, (read + d) / 1e9, d))
        del fout, wout
        torch.cuda.empty_cache()
    own = "references of its own a job"
    say(f"the ratios below: means over the {rounds} alternating rounds above")
    say(f"frames_wear against frames_trace, {own}, time per destination byte: {ratio(('frames_wear', own), ('frames_trace', own)):.3f} "
        "(expected: 1, within 15 %)")
    say(f"trace_wear against trace_flow at {w}x{h}, 4 bytes an output pixel each, time per destination byte: "
        f"{ratio(('wear', 'display'), ('flow', 'display')):.3f}")
    say(f"trace_wear (4 planes) against trace_flow (2 planes) at 224x224 floats, time per destination byte: "
        f"{ratio(('wear', '224'), ('flow', '224')):.3f}")
    say(f"memory {ctx.memory_usage()} ({'unchanged' if ctx.memory_usage() == before else 'CHANGED'})")
    ctx.close()
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
