"""Dev aid (GPU): vp8hip_trace_gather_async on n traces of p_dense_1920x1080, decoded and traced as tools/trace_time.py sets them up
(every job a one-hop trace through references of its own), every job with a source tensor of its own: float16 feature maps of 64
channels at 240x135 in both layouts with both filters, and a label map of 21 planes of bytes at the display size.  In the same run
the two yardsticks it is held against, neither of which is the code under test:
  (a) the torch formulation the call replaces, index or grid construction included, a chunk of frames at a time: for nearest cell
      indices from trace_flow(int16) and advanced indexing, for bilinear a grid from trace_flow(float32) and
      torch.nn.functional.grid_sample(align_corners=False);
  (b) trace_flow with float32 at the same output grid.
Device events around each side, 20 calls after 3; GB by the byte model: 4 bytes of trace per output, the source once, the destination.
--one-hop: the references are key frames' traces (the identity) instead of random positions, so that every job's trace is one hop of
the stream's own block motion -- piecewise constant, what a group of pictures gives -- and not a scatter over the whole picture.
   python3 tools/trace_gather_time.py [jobs (256, or as many as fit)] [timed calls (20)] [--one-hop] [--out FILE]"""
import os
import sys

import torch  # first: the library then shares torch's HIP runtime
import torch.nn.functional as F
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
sys.path.insert(0, HERE)
from rgb_time import timed  # noqa: E402
from vp8_testlib import ivf_path, load_package  # noqa: E402

CHUNK = 16              # frames per step of the torch route


def torch_nearest(ctx, pool, idx, src, out):
    """yardstick (a), nearest: out[i] = src[i] at the cell under the clamped position pool[idx[i]] names"""
    n, C, gh, gw = out.shape
    sh, sw = src.shape[2:]
    dw, dh = ctx.width, ctx.height
    size = {} if (gw, gh) == (dw, dh) else dict(width=gw, height=gh)
    sx = ((2 * torch.arange(gw, device=out.device) + 1) * dw) // (2 * gw)
    sy = ((2 * torch.arange(gh, device=out.device) + 1) * dh) // (2 * gh)
    last = src.is_contiguous(memory_format=torch.channels_last) and not src.is_contiguous()
    for i0 in range(0, n, CHUNK):
        flow = ctx.trace_flow(pool, idx[i0:i0 + CHUNK], **size).to(torch.int64)                # [c, 2, gh, gw]
        ax = (flow[:, 0] + sx[None, None, :]).clamp_(0, dw - 1)
        ay = (flow[:, 1] + sy[None, :, None]).clamp_(0, dh - 1)
        cell = (((2 * ay + 1) * sh) // (2 * dh)) * sw + ((2 * ax + 1) * sw) // (2 * dw)        # [c, gh, gw]
        s = src[i0:i0 + CHUNK]
        if last:
            rows = s.permute(0, 2, 3, 1).flatten(1, 2)                                        # [c, sh * sw, C]
            got = rows[torch.arange(rows.shape[0], device=rows.device)[:, None], cell.flatten(1)]
            out[i0:i0 + CHUNK].permute(0, 2, 3, 1).flatten(1, 2).copy_(got)
        else:
            out[i0:i0 + CHUNK] = s.flatten(2).gather(2, cell.flatten(1)[:, None, :].expand(-1, C, -1)).view(-1, C, gh, gw)


def torch_bilinear(ctx, pool, idx, src, out):
    """yardstick (a), bilinear: grid_sample at the pixel centres the traces name"""
    n, C, gh, gw = out.shape
    dw, dh = ctx.width, ctx.height
    size = {} if (gw, gh) == (dw, dh) else dict(width=gw, height=gh)
    sx = (((2 * torch.arange(gw, device=out.device) + 1) * dw) // (2 * gw)).float()
    sy = (((2 * torch.arange(gh, device=out.device) + 1) * dh) // (2 * gh)).float()
    for i0 in range(0, n, CHUNK):
        flow = ctx.trace_flow(pool, idx[i0:i0 + CHUNK], dtype=torch.float32, **size)
        ax = (flow[:, 0] + sx[None, None, :]).clamp_(0, dw - 1)
        ay = (flow[:, 1] + sy[None, :, None]).clamp_(0, dh - 1)
        grid = torch.stack(((2 * ax + 1) / dw - 1, (2 * ay + 1) / dh - 1), -1).to(src.dtype)
        out[i0:i0 + CHUNK] = F.grid_sample(src[i0:i0 + CHUNK], grid, mode="bilinear", padding_mode="border", align_corners=False)


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
    per_job = nmb * 960 + 2 * trace_bytes + 2 * 21 * w * h + 8 * w * h           # a slot, two pool entries, labels in and out, a flow tensor
    free, _ = torch.cuda.mem_get_info(0)
    n = int(args[0]) if args else min(256, int(free * 0.7) // per_job)
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
    pool = ctx.trace_pool(2 * n)
    rng = np.random.default_rng(1)
    some = torch.from_numpy(np.stack([rng.integers(0, w, (4, h, w)), rng.integers(0, h, (4, h, w))], -1).astype(np.int16)).to("cuda:0")
    one_hop = "--one-hop" in sys.argv
    if one_hop:
        ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.int16), torch.arange(w, dtype=torch.int16), indexing="ij")
        some = torch.stack((xs, ys), -1)[None].expand(4, -1, -1, -1).to("cuda:0")
    for i in range(n):                                  # the references: positions inside the picture, or the identity
        pool[i] = some[i % 4]
    del some
    ctx.frames_trace(ctx.job_array([(i, n + i, (i, (i + 1) % n, (i + 2) % n)) for i in range(n)]), pool)
    ctx.sync()
    before = ctx.memory_usage()
    say(f"p_dense_1920x1080 ({', '.join(kinds)}) x {n} jobs, a trace and a source tensor of its own each; references: "
        f"{'the identity (one hop of block motion)' if one_hop else 'random positions'}; {reps} timed calls after 3; memory {before}")
    idx = list(range(n, 2 * n))
    jobs = [(n + i, i) for i in range(n)]
    per_byte = {}

    def row(what, ms, gb, dst):
        say(f"{what:66s} {ms:9.3f} ms per call, {gb:7.2f} GB by the byte model, {gb / ms:6.3f} TB/s, {ms * 1e9 / dst:7.4f} ps per destination byte")
        return ms / dst

    cases = [((240, 135), torch.float16, 64, layout, filt) for layout in ("planar", "channels_last") for filt in ("nearest", "bilinear")]
    cases.append(((w, h), torch.uint8, 21, "planar", "nearest"))
    flow_done = set()
    for (gw, gh), dtype, C, layout, filt in cases:
        name = str(dtype).split(".")[-1]
        fmt = torch.contiguous_format if layout == "planar" else torch.channels_last
        size = {} if (gw, gh) == (w, h) else dict(width=gw, height=gh)
        model = lambda C_, es: (4 * gw * gh + 2 * C_ * gw * gh * es) * n         # noqa: E731  (trace, source once, destination)
        if (gw, gh) not in flow_done:
            flow_done.add((gw, gh))
            fl = torch.empty((n, 2, gh, gw), dtype=torch.float32, device="cuda:0")
            ms = timed(lambda: ctx.trace_flow(pool, idx, dtype=torch.float32, out=fl, **size), 3, reps)
            dst = fl[0].numel() * 4 * n
            per_byte["flow", gw] = (row(f"yardstick (b)  trace_flow {gw}x{gh} float32", ms, (4 * gw * gh * n + dst) / 1e9, dst), (4 * gw * gh * n + dst) / dst)
            del fl
        if dtype == torch.uint8:
            src = torch.randint(0, 21, (n, C, gh, gw), dtype=dtype, device="cuda:0").contiguous(memory_format=fmt)
        else:
            src = torch.empty((n, C, gh, gw), dtype=dtype, device="cuda:0").uniform_(-8, 8).contiguous(memory_format=fmt)
        out = torch.empty((n, C, gh, gw), dtype=dtype, device="cuda:0", memory_format=fmt)
        es = src.element_size()
        dst = C * gw * gh * es * n
        ms = timed(lambda: ctx.trace_gather(pool, jobs, src, filter=filt, out=out, **size), 3, reps)
        mine = row(f"trace_gather {gw}x{gh} {name} C={C} {layout} {filt}", ms, model(C, es) / 1e9, dst)
        per_byte[gw, layout, filt] = (mine, model(C, es) / dst)
        assert ctx.memory_usage() == before
        route = torch_nearest if filt == "nearest" else torch_bilinear
        ms_t = timed(lambda: route(ctx, pool, idx, src, out), 3, reps)
        row(f"yardstick (a)  torch, {CHUNK} frames a step: the same tensor", ms_t, model(C, es) / 1e9, dst)
        say(f"    yardstick (a) against trace_gather: {ms_t / ms:.1f} x the time")
        del src, out
        torch.cuda.empty_cache()
    mine, mine_model = per_byte[240, "planar", "nearest"]
    flow, flow_model = per_byte["flow", 240]
    ratio = mine_model / flow_model
    say(f"planar float16 nearest at 240x135 against yardstick (b), time per destination byte: {mine / flow:.3f} "
        f"(byte models per destination byte: {ratio:.3f}; expected: at most {ratio:.3f} x 1.25 = {1.25 * ratio:.3f}: "
        f"{'met' if mine / flow <= 1.25 * ratio else 'MISSED'})")
    say(f"memory {ctx.memory_usage()} ({'unchanged' if ctx.memory_usage() == before else 'CHANGED'})")
    ctx.close()
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
