"""Dev aid (GPU): vp8hip_frames_trace_async and vp8hip_trace_flow_async on a batch of IR slots holding p_dense_1920x1080's key frame
and three inter frames, over and over -- and, in the same run, the yardstick they are held against, which is not the code under
test: frames_side for the same slots with int16 vectors and no planes at 1920x1080 (the same 4 bytes a pixel written), and with
floats at 224x224 for the flow tensor.  Every job has references of its own (entries i, i + 1, i + 2 of the pool's first half, the
destinations in the second), so that what a hop gathers comes from HBM as it would for streams in lock step.  Device events around
each call after warm-up; TB/s by the byte model: records (128 bytes a macroblock: the line the dword read lies in) and vectors (64)
read, one gathered dword a pixel (no gather for a key frame), plus the destination bytes.
   python3 tools/trace_time.py [slots (4096, or as many as fit beside the pool)] [timed calls (20)] [--out FILE]"""
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
    trace_bytes = P.trace_size(w, h)
    per_frame = nmb * 960 + 2 * trace_bytes             # a slot, a reference entry and a destination entry of the pool
    free, _ = torch.cuda.mem_get_info(0)
    n = int(args[0]) if args else min(4096, int(free * 0.9) // per_frame)
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
    slots = list(range(n))
    n_inter = sum(kinds[i % len(kinds)] == "inter" for i in range(n))
    src_side = nmb * (128 + 64)
    per_byte = {}

    def row(what, ms, gb, dst):
        say(f"{what:52s} {ms:8.3f} ms per call, {gb:7.2f} GB by the byte model, {gb / ms:6.3f} TB/s, {ms * 1e9 / dst:7.4f} ps per destination byte")
        return ms / dst

    for (gw, gh), dtype, key in (((w, h), torch.int16, "side"), ((224, 224), torch.float32, "side224")):
        mv = torch.empty((n, 2, gh, gw), dtype=dtype, device="cuda:0")
        ms = timed(lambda: ctx.frames_side(slots, gw, gh, mv_dtype=dtype, planes=(), scale=None if dtype == torch.int16 else "pixels", out_mv=mv), 3, reps)
        dst = mv[0].numel() * mv.element_size() * n
        per_byte[key] = row(f"yardstick  frames_side {gw}x{gh} mv {str(dtype).split('.')[-1]} + 0 planes", ms, (src_side * n + dst) / 1e9, dst)
        del mv
        torch.cuda.empty_cache()

    pool = ctx.trace_pool(2 * n)
    rng = np.random.default_rng(1)
    some = torch.from_numpy(np.stack([rng.integers(0, w, (4, h, w)), rng.integers(0, h, (4, h, w))], -1).astype(np.int16)).to("cuda:0")
    for i in range(n):                                  # the references: positions inside the picture
        pool[i] = some[i % 4]
    del some
    jobs = ctx.job_array([(i, n + i, (i, (i + 1) % n, (i + 2) % n)) for i in range(n)])
    ms = timed(lambda: ctx.frames_trace(jobs, pool), 3, reps)
    dst = trace_bytes * n
    per_byte["trace"] = row(f"frames_trace {w}x{h}, references of its own a job", ms, (src_side * n + trace_bytes * n_inter + dst) / 1e9, dst)
    shared = ctx.job_array([(i, n + i, (0, 1, 2)) for i in range(n)])
    ms = timed(lambda: ctx.frames_trace(shared, pool), 3, reps)
    row(f"frames_trace {w}x{h}, three references for all jobs", ms, (src_side * n + dst) / 1e9, dst)
    keys = ctx.job_array([(i - i % len(kinds), n + i, None) for i in range(n)])
    ms = timed(lambda: ctx.frames_trace(keys, pool), 3, reps)
    row(f"frames_trace {w}x{h}, key frames only (the identity)", ms, dst / 1e9, dst)
    ctx.frames_trace(jobs, pool)

    idx = list(range(n, 2 * n))
    for (gw, gh), dtype, key in (((224, 224), torch.float32, "flow224"), ((w, h), torch.int16, "flow")):
        free, _ = torch.cuda.mem_get_info(0)
        m = min(n, int(free * 0.8) // (2 * gh * gw * 4))
        out = torch.empty((m, 2, gh, gw), dtype=dtype, device="cuda:0")
        size = {} if (gw, gh) == (w, h) else dict(width=gw, height=gh)
        ms = timed(lambda: ctx.trace_flow(pool, idx[:m], dtype=dtype, scale=None if dtype == torch.int16 else "pixels", out=out, **size), 3, reps)
        dst = out[0].numel() * out.element_size() * m
        read = min(gw * gh, w * h) * 4 * m              # (a small grid touches a dword per output)
        per_byte[key] = row(f"trace_flow {gw}x{gh} {str(dtype).split('.')[-1]}, {m} entries", ms, (read + dst) / 1e9, dst)
        del out
        torch.cuda.empty_cache()
    say(f"frames_trace against frames_side at {w}x{h} int16, time per destination byte: {per_byte['trace'] / per_byte['side']:.3f} "
        "(byte model: 1.84; every gathered piece on two sectors: 2.7; expected: at most 2.7 x 1.15)")
    say(f"trace_flow against frames_side at 224x224 floats, time per destination byte: {per_byte['flow224'] / per_byte['side224']:.3f}")
    say(f"memory {ctx.memory_usage()} ({'unchanged' if ctx.memory_usage() == before else 'CHANGED'})")
    ctx.close()
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
