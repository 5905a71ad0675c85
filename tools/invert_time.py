"""Dev aid (GPU): vp8hip_trace_invert_async over tools/trace_time.py's pool -- the traces of a batch of IR slots holding
p_dense_1920x1080's key frame and three inter frames, every job with references of its own (of random positions, so that a trace
scatters over the whole picture) -- FIRST only, COUNT only and both, and vp8hip_trace_cover_async over the COUNT entries; and, in
the same process, the yardsticks they are held against, which are not the code under test: trace_flow int16 at the display size
over the same entries (the same bytes in and out as a FIRST-only call), and the torch formulation the call replaces (the indices
built from the trace, scatter_reduce_(amin), bincount; a frame at a time, over a few entries).  The same jobs through key frames'
traces give one hop of the stream's block motion.  Controls: a pool of identity traces (every atomic of a wave on consecutive
dwords, no two on one) and a constant trace (every pixel on one anchor pixel: full contention; a handful of entries).  The sides
of a comparison alternate A B B A.
Device events around each call after warm-up; atomic bytes = 4 per pixel and output.
   python3 tools/invert_time.py [entries (4096, or as many as fit)] [timed calls (20)] [--out FILE]"""
import os
import sys

import torch  # first: the library then shares torch's HIP runtime
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
sys.path.insert(0, HERE)
from rgb_time import timed  # noqa: E402
from vp8_testlib import ivf_path, load_package  # noqa: E402


def torch_invert(pool, entries, w, h, first, count):
    """the formulation the call replaces, a frame at a time: -> nothing; first [m, h * w] int32 (signed amin: positions are below
    2^30, "none" is the int32 maximum here), count [m, h * w] int64"""
    own = (torch.arange(h, device=pool.device, dtype=torch.int32)[:, None] << 16 | torch.arange(w, device=pool.device, dtype=torch.int32)[None, :]).flatten()
    for k, e in enumerate(entries):
        t = pool[e].to(torch.int64)
        a = (t[..., 1].clamp_(0, h - 1) * w + t[..., 0].clamp_(0, w - 1)).flatten()
        first[k].fill_(0x7fffffff).scatter_reduce_(0, a, own, "amin")
        count[k] = torch.bincount(a, minlength=h * w)


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
    per_frame = nmb * 960 + 5 * entry                   # a slot; a reference and a destination trace; FIRST, COUNT, the yardstick's tensor
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
    say(f"p_dense_1920x1080 ({', '.join(kinds)}) x {n} slots; {reps} timed calls after 3")
    rng = np.random.default_rng(1)
    pool = ctx.trace_pool(2 * n)
    some = torch.from_numpy(np.stack([rng.integers(0, w, (4, h, w)), rng.integers(0, h, (4, h, w))], -1).astype(np.int16)).to("cuda:0")
    for i in range(n):                                  # the references: positions inside the picture
        pool[i] = some[i % 4]
    chained = ctx.job_array([(i, n + i, (i, (i + 1) % n, (i + 2) % n)) for i in range(n)])
    keys = ctx.job_array([(i - i % len(kinds), n + i, None) for i in range(n)])
    ctx.frames_trace(chained, pool)
    first, count = ctx.cover_pools(n)
    flow = torch.empty((n, 2, h, w), dtype=torch.int16, device="cuda:0")
    ctx.sync()
    before = ctx.memory_usage()
    idx = list(range(n, 2 * n))
    jobs = [(n + i, i) for i in range(n)]
    per = {}

    def row(key, what, ms, entries, outputs):
        gb = 4 * w * h * entries * outputs / 1e9
        say(f"{what:64s} {ms:9.3f} ms per call, {ms * 1e3 / entries:9.3f} us an entry" +
            (f", {gb:6.2f} GB of atomics, {gb / ms:6.3f} TB/s" if outputs else ""))
        per.setdefault(key, []).append(ms / entries)

    def ratio(a, b):
        return (sum(per[a]) / len(per[a])) / (sum(per[b]) / len(per[b]))

    def yardstick(tag, which):
        row(("flow", which, tag), f"yardstick  trace_flow {w}x{h} int16, {n} entries ({tag})", timed(lambda: ctx.trace_flow(pool, idx, out=flow), 3, reps), n, 0)

    def invert(tag, which, f, c, js=jobs, warm=3, r=reps):
        row((which, tag), f"trace_invert {which}, {len(js)} entries ({tag})", timed(lambda: ctx.trace_invert(pool, js, f, c), warm, r), len(js),
            (f is not None) + (c is not None))

    anchors = ctx.job_array([(i - i % len(kinds), i, None) for i in range(n)])       # the identity into the references' entries
    for tag, fill in (("traces of the stream", chained), ("identity traces", keys), ("one hop of block motion", chained)):
        if tag == "one hop of block motion":            # the same jobs through key frames' traces: what a stream's second frame has
            ctx.frames_trace(anchors, pool)
        ctx.frames_trace(fill, pool)
        # A B B A: yardstick, call, call, yardstick -- per output set
        for which, f, c in (("FIRST", first, None), ("COUNT", None, count), ("both", first, count)):
            yardstick(tag, which)
            invert(tag, which, f, c)
            invert(tag, which, f, c)
            yardstick(tag, which)
    # full contention: every pixel on one anchor pixel, a handful of entries
    few = 4
    pool[n:n + few] = 0
    pool[n:n + few, :, :, 0] = w // 2
    pool[n:n + few, :, :, 1] = h // 2
    for which, f, c in (("FIRST", first, None), ("COUNT", None, count), ("both", first, count)):
        invert("a constant trace", which, f, c, jobs[:few], 1, 3)
    for i in range(n):                                  # the references scattered again, as they were
        pool[i] = some[i % 4]
    del some
    ctx.frames_trace(chained, pool)
    ctx.trace_invert(pool, jobs, first, count)

    # the tensor of the COUNT entries against the flow tensor of the same size and bytes out (2 planes of bytes / 2 planes of int16)
    cover = torch.empty((n, 2, h, w), dtype=torch.uint8, device="cuda:0")
    for _ in range(2):
        row(("cover", "display"), f"trace_cover {w}x{h} uint8, 2 planes, {n} entries", timed(lambda: ctx.trace_cover(count, list(range(n)), out=cover), 3, reps), n, 0)
    del cover

    # the torch formulation, over a few entries (a frame at a time, as a caller would write it)
    m = min(n, 32)
    tf = torch.empty((m, h * w), dtype=torch.int32, device="cuda:0")
    tc = torch.empty((m, h * w), dtype=torch.int64, device="cuda:0")
    tag = "traces of the stream"
    for order in ("AB", "BA"):
        for side in order:
            if side == "A":
                row(("torch", tag), f"yardstick  torch: indices, scatter_reduce_(amin), bincount, {m} entries", timed(lambda: torch_invert(pool, idx[:m], w, h, tf, tc), 1, 3), m, 0)
            else:
                invert(tag + f", {m} entries", "both", first, count, jobs[:m])
    same = bool((tc.to(torch.int32) == count[:m].flatten(1)).all()) and bool(
        (torch.where(tf == 0x7fffffff, torch.full_like(tf, -1), tf) == first[:m].view(torch.int32).flatten(1)).all())
    say(f"the torch formulation and trace_invert agree on those {m} entries: {same}")
    say("the ratios below: means over the alternating rounds above, time per entry")
    for kind in ("traces of the stream", "identity traces", "one hop of block motion"):
        for which in ("FIRST", "COUNT", "both"):
            say(f"trace_invert {which} against trace_flow int16 at {w}x{h}, {kind}: {ratio((which, kind), ('flow', which, kind)):.3f}")
    for which in ("FIRST", "COUNT", "both"):
        say(f"trace_invert {which}, a constant trace against traces of the stream: {ratio((which, 'a constant trace'), (which, 'traces of the stream')):.1f}")
    say(f"trace_invert both against the torch formulation, {m} entries: {ratio(('both', tag + f', {m} entries'), ('torch', tag)):.4f}")
    say(f"trace_cover uint8 (2 planes) against trace_flow int16 (2 planes) at {w}x{h}: {ratio(('cover', 'display'), ('flow', 'both', tag)):.3f}")
    say(f"memory {ctx.memory_usage()} ({'unchanged' if ctx.memory_usage() == before else 'CHANGED'})")
    ctx.close()
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
