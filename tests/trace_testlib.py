"""What the tests of the trace calls share: frames and their restated traces (CPU), a trace to and from a pool on the device (GPU)."""
import numpy as np

from vp8_testlib import ivf_path
import trace_reference as R

NEARESTMV, NEARMV, ZEROMV, NEWMV, SPLITMV = 5, 6, 7, 8, 9


def make_hdr(P, w, h, frame_type=1):
    hdr = P.FrameHdr()
    hdr.width, hdr.height, hdr.mb_cols, hdr.mb_rows, hdr.frame_type = w, h, (w + 15) // 16, (h + 15) // 16, frame_type
    hdr.show_frame = 1
    return hdr


def luma(buf, g, h, w, border=0):
    o = g.y_off - border * g.y_stride - border
    return np.lib.stride_tricks.as_strided(buf[o:], shape=(h + 2 * border, w + 2 * border), strides=(g.y_stride, 1))


def whole_pixel_frame(P, w, h, rng):
    """every macroblock inter and skipped, references 1..3 mixed, whole-pixel vectors that take a block at most 24 pixels past any
    edge of the coded area, a third of the macroblocks SPLITMV (all four partitionings)"""
    hdr = make_hdr(P, w, h)
    cols, rows = hdr.mb_cols, hdr.mb_rows
    nmb = cols * rows
    mbs = np.zeros((nmb, 64), np.uint8)
    mvs = np.zeros((nmb, 16, 2), np.int16)
    mbs[:, 3] = 1                                # skipped: no residual
    split = [np.repeat(np.arange(2), 8), np.tile(np.repeat(np.arange(2), 2), 4), (np.arange(16) // 8) * 2 + (np.arange(16) % 4) // 2, np.arange(16)]
    for i in range(nmb):
        r, c = divmod(i, cols)
        mbs[i, 2] = rng.integers(1, 4)
        lo_x, hi_x = max(-24 - 16 * c, -48), min(16 * (cols - 1 - c) + 24, 48)
        lo_y, hi_y = max(-24 - 16 * r, -48), min(16 * (rows - 1 - r) + 24, 48)

        def vec(n):
            return np.stack([rng.integers(lo_y, hi_y + 1, n), rng.integers(lo_x, hi_x + 1, n)], 1) * 8
        if i % 3 == 0:
            part = 3 if nmb == 1 else int(rng.integers(0, 4))          # (a lone macroblock: sixteen vectors)
            mbs[i, 0], mbs[i, 5] = SPLITMV, part
            mvs[i] = vec(16)[split[part]]
        else:
            mbs[i, 0] = NEWMV
            mvs[i] = vec(1)
    return hdr, mbs, mvs


def frames_of(P, name):
    """every frame of a fixture through the host parser: (hdr, mbs, mvs, (new, last, golden, alt) as vp8_refs numbers them)"""
    _, _, frames = P.read_ivf(ivf_path(name))
    parser = P.Parser()
    out = []
    try:
        for data in frames:
            hdr, _, mbs, _, mvs = P.parse_to_numpy(parser, data)
            r = parser.refs
            out.append((hdr, mbs, mvs, (r.new_idx, r.lst_idx, r.gld_idx, r.alt_idx)))
            parser.swap(hdr)
    finally:
        parser.close()
    return out


def chain(frames, last_only=False):
    """the trace of every frame, the pool numbered like the frame buffers; last_only: every macroblock follows the last frame"""
    pool, out = {}, []
    for hdr, mbs, mvs, (new, lst, gld, alt) in frames:
        if last_only:
            mbs = mbs.copy()
            mbs[:, R.O_REF] = np.minimum(mbs[:, R.O_REF], 1)
            gld = alt = None
        pool[new] = R.trace(hdr, mbs, mvs, [pool.get(lst), pool.get(gld), pool.get(alt)])
        out.append(pool[new])
    return out


def slot_ir(ctx, slot):
    return ctx.ir_fetch(slot)[0], ctx.mvs_fetch(slot)


def dwords(t):
    """a pool or entries of one on the device -- int16 [..., h, w, 2], uint8 [..., h, w, 4] or int32 [..., h, w] -> numpy uint32
    [..., h, w]"""
    a = np.ascontiguousarray(t.cpu().numpy())
    return a.view(np.uint32).reshape(a.shape if a.itemsize == 4 else a.shape[:-1])


def to_pool(a, dtype=np.int16):
    """numpy uint32 [h, w] -> a pool entry of elements `dtype` on the device: int16 [h, w, 2], uint8 [h, w, 4] or int32 [h, w]"""
    import torch
    per = 4 // np.dtype(dtype).itemsize
    return torch.from_numpy(np.ascontiguousarray(a).view(dtype).reshape(a.shape + ((per,) if per > 1 else ()))).to("cuda:0")


def scales(n, scale):
    """a call's scale argument -- None, one number or n -- as the n numbers the restatements take"""
    return (1.0,) * n if scale is None else (scale,) * n if np.ndim(scale) == 0 else scale


def check_tensor(call, tensor, nscale, ctx, pool, idx, want, dw, dh, dtype, planes, scale, what=None, **kw):
    """entries idx of the pool through Vp8Hip's `call` (trace_wear, trace_cover) against the restatement `tensor` (wear_reference's,
    invert_reference's) on `want` (what the entries hold, numpy)"""
    from handover_testlib import TORCH_DTYPE, bits
    size = {} if dw == 0 else dict(width=dw, height=dh)
    got = getattr(ctx, call)(pool, idx, planes=planes, dtype=TORCH_DTYPE[dtype], scale=scale, **size, **kw).cpu().numpy()
    assert got.shape[0] == len(idx)
    for k, t in enumerate(want):
        ref = tensor(t, dw, dh, planes, dtype, scales(nscale, scale))
        assert got[k].shape == ref.shape and np.array_equal(bits(got[k], dtype), bits(ref, dtype)), (what, k, dw, dh, dtype, planes, scale)


def random_trace(rng, w, h):
    """seeded random positions inside the picture"""
    return R.pack(rng.integers(0, w, (h, w)), rng.integers(0, h, (h, w)))


def traced_stream(P, name, form, monkeypatch):
    """every frame of a fixture into a frame buffer of its own and traced into the pool entry of that number, one launch per frame;
    -> (ctx, pool, traces by trace_reference over the slot's IR, shown frames, frame types)"""
    monkeypatch.setenv("VP8HIP_RECON", "simt" if form == "tiles" else "wave")
    w, h, frames = P.read_ivf(ivf_path(name))
    nf = len(frames)
    ctx = P.Vp8Hip(0)
    parser = P.Parser()
    try:
        ctx.configure(w, h, nf + 1, 1)
        pool = ctx.trace_pool(nf + 1)
        pool.zero_()
        mine = [None] * nf + [np.zeros((h, w), np.uint32)]
        phys, shown, types = {}, [], []
        for i, data in enumerate(frames):
            hdr, _ = ctx.parse_into_slot_compact(parser, data, 0)
            r = parser.refs
            refs = tuple(phys.get(k, nf) for k in (r.lst_idx, r.gld_idx, r.alt_idx))
            ctx.decode([(0, i, refs)], P.STAGE_ALL)
            ctx.frames_trace([(0, i, refs)], pool)
            ctx.sync()
            mbs, mvs = slot_ir(ctx, 0)
            mine[i] = R.trace(hdr, mbs, mvs, [mine[k] for k in refs])
            new = r.new_idx
            parser.swap(hdr)
            phys[new] = i
            types.append(hdr.frame_type)
            if hdr.show_frame:
                shown.append(phys[parser.refs.show_idx])
    except BaseException:
        ctx.close()
        raise
    finally:
        parser.close()
    return ctx, pool, mine, shown, types
