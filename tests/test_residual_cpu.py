"""CPU: tests/residual_reference.py -- the numpy restatement of vp8hip_frames_residual_async's definition (include/vp8hip.h) that the
GPU tests compare with bit for bit -- pinned to the oracle, plus the library's size function through ctypes and the grid maps.

What pins what.  The oracle never hands out the residual itself, only pixels, clamp255(prediction + R), and the int16 outputs of
its dequantiser and its two inverse Walsh transforms.  So:
  * inter macroblocks, whole frames: their prediction depends on nothing in their own frame, so a second decode with every
    macroblock skipped gives it, and clamp255(pred + R) == rec pins every sample with |R| <= 255 -- on the fixtures all of them;
  * intra 16x16 luma and all intra chroma: the same with one macroblock skipped at a time (its neighbours are unchanged);
  * B_PRED luma, whose sub-blocks predict from each other, and the range beyond +-255: blocks by themselves through the oracle's
    block functions over flat predictors 0 and 255, which give clip(R, -255, 255) exactly, and through vp8o_dequantize_b and
    vp8o_short_inv_walsh4x4 / _1, whose int16 outputs are compared bit for bit -- with coefficients of +-2047 and the largest
    factors, where the int16 truncations bite.
Beyond +-255 the reference's behaviour is observable only through those int16 outputs and through clamped pixels: there the C
semantics stated in include/vp8hip.h are the definition, and residual_reference.py is their second statement."""
import ctypes
import itertools

import numpy as np
import pytest

from vp8_testlib import ivf_path, oracle, oracle_decode, random_frame, synth_ir
import residual_reference as R

STAGE_RECON = 1
# synth_ir seeds (seed, inter) whose quantisers keep nearly all of the residual within +-255 at 48x32 and 67x45
SYNTH_SEEDS = ((40, False), (54, False), (117, False), (291, False), (40, True), (54, True))
B_PRED, SPLITMV = 4, 9


def plane_views(P, buf, g):
    """the coded area of a frame buffer: (Y, U, V) as int64"""
    def view(off, stride, w, h):
        return np.lib.stride_tricks.as_strided(buf[off:], shape=(h, w), strides=(stride, 1)).astype(np.int64)
    return (view(g.y_off, g.y_stride, g.aligned_w, g.aligned_h), view(g.u_off, g.uv_stride, g.aligned_w // 2, g.aligned_h // 2),
            view(g.v_off, g.uv_stride, g.aligned_w // 2, g.aligned_h // 2))


def recon(P, hdr, mbs, coef, mvs, refs, g):
    buf = np.zeros(g.frame_size, np.uint8)
    oracle_decode(hdr, mbs, coef, mvs, buf, refs, STAGE_RECON)
    return plane_views(P, buf, g)


@pytest.mark.parametrize("name", ["p_split_352x288", "p_seg_176x144", "p_odd_130x98"])
def test_inter_macroblocks_of_whole_frames(pkg, name):
    P = pkg
    _, _, frames = P.read_ivf(ivf_path(name))
    parser = P.Parser()
    checked = 0
    try:
        for i, data in enumerate(frames[:6]):
            hdr, changed, mbs, coef, mvs = P.parse_to_numpy(parser, data)
            if changed:
                g = P.geom(hdr.width, hdr.height)
                bufs = [np.zeros(g.frame_size, np.uint8) for _ in range(4)]
            r = parser.refs
            refs = (bufs[r.lst_idx], bufs[r.gld_idx], bufs[r.alt_idx])
            inter = (mbs[:, R.O_REF] != 0).reshape(hdr.mb_rows, hdr.mb_cols)
            if inter.any():
                rec = recon(P, hdr, mbs, coef, mvs, refs, g)
                skipped = mbs.copy()
                skipped[:, R.O_FLAGS] |= R.MB_SKIP
                pred = recon(P, hdr, skipped, np.zeros_like(coef), mvs, refs, g)
                res = R.residual_planes(hdr, mbs, coef)
                for a, b, d, s in zip(rec, pred, res, (16, 8, 8)):
                    m = inter.repeat(s, 0).repeat(s, 1)
                    d = d.astype(np.int64)
                    assert np.abs(d[m]).max() <= 255, (name, i)          # so the pixels pin every sample
                    assert np.array_equal(np.clip(b + d, 0, 255)[m], a[m]), (name, i)
                    checked += int(m.sum())
                # the same planes, laid out: at the display size both layouts are a crop of the coded area
                w, h = hdr.width, hdr.height
                planar = R.arrange(res, hdr, w, h, "i16", "planar")
                assert np.array_equal(planar[0], res[0][:h, :w]) and np.array_equal(planar[1], res[1].repeat(2, 0).repeat(2, 1)[:h, :w])
                flat = R.arrange(res, hdr, w, h, "i16", "i420")
                y, u, v = P.split_residual(flat, w, h)
                assert np.array_equal(y, res[0][:h, :w]) and np.array_equal(v, res[2][:(h + 1) // 2, :(w + 1) // 2])
                assert flat.nbytes == R.size(hdr, w, h, "i16", "i420") and planar.nbytes == R.size(hdr, w, h, "i16", "planar")
            oracle_decode(hdr, mbs, coef, mvs, bufs[r.new_idx], refs)
            parser.swap(hdr)
    finally:
        parser.close()
    assert checked > 4000


def _one_at_a_time(P, hdr, mbs, coef, mvs, refs, g, tally):
    """every intra macroblock that is not skipped: its 16x16 luma (not B_PRED) and its chroma against a decode that skips it alone"""
    rec = recon(P, hdr, mbs, coef, mvs, refs, g)
    res = [d.astype(np.int64) for d in R.residual_planes(hdr, mbs, coef)]
    cols = hdr.mb_cols
    for i in np.flatnonzero((mbs[:, R.O_REF] == 0) & ((mbs[:, R.O_FLAGS] & R.MB_SKIP) == 0)):
        one = mbs.copy()
        one[i, R.O_FLAGS] |= R.MB_SKIP
        pred = recon(P, hdr, one, coef, mvs, refs, g)
        r, c = divmod(int(i), cols)
        for k, s in ((0, 16), (1, 8), (2, 8)):
            if k == 0 and mbs[i, R.O_Y_MODE] == B_PRED:
                continue
            win = (slice(r * s, r * s + s), slice(c * s, c * s + s))
            d = res[k][win]
            assert np.array_equal(np.clip(pred[k][win] + d, 0, 255), rec[k][win]), (int(i), k)
            tally["samples"] += d.size
            tally["beyond"] += int((np.abs(d) > 255).sum())
        tally["mbs"] += 1
        tally["luma"] += mbs[i, R.O_Y_MODE] != B_PRED


def test_intra_16x16_luma_and_all_intra_chroma(pkg):
    P = pkg
    tally = dict(mbs=0, luma=0, samples=0, beyond=0)
    # the fixtures' key frames are almost all B_PRED: their chroma, and the few 16x16 macroblocks
    _, _, frames = P.read_ivf(ivf_path("p_seg_176x144"))
    parser = P.Parser()
    try:
        hdr, _, mbs, coef, mvs = P.parse_to_numpy(parser, frames[0])
    finally:
        parser.close()
    g = P.geom(hdr.width, hdr.height)
    _one_at_a_time(P, hdr, mbs, coef, mvs, (None, None, None), g, tally)
    assert tally["mbs"] >= 30
    # random frames have many 16x16 macroblocks (seeds whose quantisers keep nearly all of the residual within +-255)
    for (w, h), (seed, inter) in itertools.product(((48, 32), (67, 45)), SYNTH_SEEDS):
        hdr, mbs, coef, mvs = synth_ir(w, h, seed, inter=inter, big=False)
        g = P.geom(w, h)
        refs = tuple(random_frame(g, seed + k) for k in (1, 2, 3)) if inter else (None, None, None)
        _one_at_a_time(P, hdr, mbs, coef, mvs, refs, g, tally)
    assert tally["luma"] >= 30, tally
    assert tally["beyond"] * 100 <= tally["samples"], tally


def _raster(block):
    """a block of the IR (column-major) in the reference's order, and back"""
    return np.ascontiguousarray(np.asarray(block).reshape(4, 4).T).reshape(16)


def test_blocks_by_themselves(pkg):
    """every block of random macroblocks (Y2, B_PRED, SPLITMV; coefficients up to +-2047) through the oracle's block functions as
    decode_macroblock calls them, over flat predictors 0 and 255: clip(R, -255, 255), and the int16 outputs bit for bit"""
    P = pkg
    O = oracle()
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    O.vp8o_dequantize_b.argtypes = [vp, vp, vp]
    O.vp8o_short_inv_walsh4x4.argtypes = [vp, vp]
    O.vp8o_short_inv_walsh4x4_1.argtypes = [vp, vp]
    O.vp8o_dequant_idct_add.argtypes = [vp, vp, vp, i32]
    O.vp8o_dc_only_idct_add.argtypes = [ctypes.c_short, vp, i32, vp, i32]
    O.vp8o_dequant_idct_add_y_block.argtypes = [vp, vp, vp, i32, vp]
    O.vp8o_dequant_idct_add_uv_block.argtypes = [vp, vp, vp, vp, i32, vp]
    O.vp8o_mb_dequant.argtypes = [vp, i32, vp]
    bit, wrapped, n_y2 = 0, 0, [0, 0]
    for seed, qindex in ((1, 127), (2, None), (3, 127), (4, 0), (5, None)):
        hdr, mbs, coef, _ = synth_ir(64, 48, seed, inter=seed % 2 == 1, big=True, dense=0.6)
        if qindex is not None:
            hdr.segmentation_enabled, hdr.base_qindex = 0, qindex
        nmb = hdr.mb_rows * hdr.mb_cols
        blocks = R.residual_blocks(hdr, mbs, coef)
        wrapped += int((blocks != R.residual_blocks(hdr, mbs, coef, wrap=False)).sum())
        f = R.factors(hdr)
        for i in range(nmb):
            seg = int(mbs[i, R.O_SEGMENT])
            dq = (ctypes.c_short * 6)()
            O.vp8o_mb_dequant(ctypes.byref(hdr), seg, dq)
            assert list(dq) == f[seg].tolist()                              # vp8o_mb_dequant: y1, y2, uv as (dc, ac)
            if mbs[i, R.O_FLAGS] & R.MB_SKIP:
                assert not blocks[i].any()
                continue
            q = np.concatenate([_raster(coef[i, b * 16:b * 16 + 16]) for b in range(25)]).astype(np.int16)
            eobs = mbs[i, R.O_EOBS:R.O_EOBS + 25].astype(np.int8)
            y_mode = mbs[i, R.O_Y_MODE]

            def factors16(dc, ac):
                return np.array([dc] + [ac] * 15, np.int16)
            dqy = factors16(f[seg, 0], f[seg, 1])
            if y_mode not in (B_PRED, SPLITMV):                              # decodframe.c:258-284
                y2 = np.zeros(16, np.int16)
                dcs = np.zeros(256, np.int16)
                if eobs[24] > 1:
                    O.vp8o_dequantize_b(q[384:].ctypes.data, factors16(f[seg, 2], f[seg, 3]).ctypes.data, y2.ctypes.data)
                    assert np.array_equal(y2, R.s16(q[384:].astype(np.int64) * factors16(f[seg, 2], f[seg, 3])))
                    O.vp8o_short_inv_walsh4x4(y2.ctypes.data, dcs.ctypes.data)
                    assert np.array_equal(dcs[::16].reshape(4, 4), R.inv_walsh(y2.astype(np.int64).reshape(4, 4)))
                else:
                    y2[0] = R.s16(int(q[384]) * int(f[seg, 2]))
                    O.vp8o_short_inv_walsh4x4_1(y2.ctypes.data, dcs.ctypes.data)
                n_y2[int(eobs[24] > 1)] += 1
                # ... the DCs are where residual_blocks has them: a luma block with eob <= 1 is its DC alone
                for b in range(16):
                    if eobs[b] <= 1:
                        assert (blocks[i, b] == (int(dcs[16 * b]) + 4) >> 3).all()
                bit += 16
                q[0:256:16] = dcs[::16]
                dqy = factors16(1, f[seg, 1])
            clip = np.zeros((2, 24, 4, 4), np.int64)
            for k, flat in enumerate((0, 255)):
                ybuf = np.full((16, 16), flat, np.uint8)
                ubuf, vbuf = np.full((8, 8), flat, np.uint8), np.full((8, 8), flat, np.uint8)
                qq = q.copy()
                if y_mode == B_PRED:                                        # decodframe.c:200-236: block by block
                    for b in range(16):
                        d = ybuf[(b >> 2) * 4:, (b & 3) * 4:]
                        if eobs[b] > 1:
                            O.vp8o_dequant_idct_add(qq[16 * b:].ctypes.data, dqy.ctypes.data, d.ctypes.data, 16)
                        elif eobs[b]:
                            O.vp8o_dc_only_idct_add(int(R.s16(int(qq[16 * b]) * int(dqy[0]))), d.ctypes.data, 16, d.ctypes.data, 16)
                else:
                    O.vp8o_dequant_idct_add_y_block(qq.ctypes.data, dqy.ctypes.data, ybuf.ctypes.data, 16, eobs.ctypes.data)
                O.vp8o_dequant_idct_add_uv_block(qq[256:].ctypes.data, factors16(f[seg, 4], f[seg, 5]).ctypes.data, ubuf.ctypes.data, vbuf.ctypes.data,
                                                 8, eobs[16:].ctypes.data)
                clip[k, :16] = ybuf.astype(np.int64).reshape(4, 4, 4, 4).transpose(0, 2, 1, 3).reshape(16, 4, 4) - flat
                clip[k, 16:20] = ubuf.astype(np.int64).reshape(2, 4, 2, 4).transpose(0, 2, 1, 3).reshape(4, 4, 4) - flat
                clip[k, 20:24] = vbuf.astype(np.int64).reshape(2, 4, 2, 4).transpose(0, 2, 1, 3).reshape(4, 4, 4) - flat
            want = blocks[i]
            assert np.array_equal(clip[0], np.clip(want, 0, 255)) and np.array_equal(clip[1], np.clip(want, -255, 0)), (seed, i)
            assert np.array_equal(clip[0] + clip[1], np.clip(want, -255, 255))
    assert wrapped > 0 and bit > 0 and min(n_y2) > 0


def test_walsh_and_dequantiser_at_the_extremes():
    """the two int16 functions on inputs the frames above may not reach: every coefficient +-2047 against every largest factor"""
    O = oracle()
    O.vp8o_dequantize_b.argtypes = [ctypes.c_void_p] * 3
    O.vp8o_short_inv_walsh4x4.argtypes = [ctypes.c_void_p] * 2
    O.vp8o_short_inv_walsh4x4_1.argtypes = [ctypes.c_void_p] * 2
    rng = np.random.default_rng(9)
    changed = 0
    for _ in range(300):
        q = rng.choice(np.array([-2047, 2047, -2048, 0, 1, -1, 1024], np.int16), 16)
        dqc = np.array([int(rng.choice([314, 8, 157 * 2]))] + [int(rng.choice([440, 8, 284]))] * 15, np.int16)
        dq, out = np.zeros(16, np.int16), np.zeros(256, np.int16)
        O.vp8o_dequantize_b(q.ctypes.data, dqc.ctypes.data, dq.ctypes.data)
        want = R.s16(q.astype(np.int64) * dqc)
        assert np.array_equal(dq, want)
        changed += int((want != q.astype(np.int64) * dqc).sum())
        O.vp8o_short_inv_walsh4x4(dq.ctypes.data, out.ctypes.data)
        w = R.inv_walsh(want.reshape(4, 4))
        assert np.array_equal(out[::16].reshape(4, 4), w)
        changed += int((w != R.inv_walsh(want.reshape(4, 4), R.keep)).sum())
        O.vp8o_short_inv_walsh4x4_1(dq.ctypes.data, out.ctypes.data)
        assert (out[::16] == R.s16((int(dq[0]) + 3) >> 3)).all()
    assert changed > 0


def test_size_function_of_the_library(pkg):
    P = pkg
    L = P.load_hip()

    def lib(w, h, layout=1, dtype=0):
        p = P.ResidualParams(w, h, layout, dtype)
        return int(L.vp8hip_residual_size(None, ctypes.byref(p)))
    hdr = P.FrameHdr()
    hdr.width, hdr.height, hdr.mb_cols, hdr.mb_rows = 64, 48, 4, 3
    for (w, h), (dt, name), (lay, lname) in itertools.product(((1, 1), (224, 224), (1920, 1080), (16383, 16383), (7, 3), (16383, 1), (130, 98)),
                                                             enumerate(("i16", "f16", "f32")), enumerate(("i420", "planar"))):
        want = R.size(hdr, w, h, name, lname)
        assert lib(w, h, lay, dt) == want, (w, h, name, lname)
        assert P.residual_sizes(w, h, dt, lname) == want
    assert lib(7, 3, 0, 0) == (21 + 2 * 4 * 2) * 2 and lib(7, 3, 1, 2) == 3 * 21 * 4
    assert R.size(hdr) == 3 * 64 * 48 * 2 and R.size(hdr, layout="i420") == (64 * 48 + 2 * 32 * 24) * 2       # the native grid
    # everything the call refuses on the parameters alone: zero
    for w, h in ((0, 5), (5, 0), (16384, 2), (2, 16384), (-1, -1), (-3, 5)):
        assert lib(w, h) == 0 and lib(w, h, 0, 2) == 0, (w, h)
        assert P.residual_sizes(w, h) == 0
    for dt in (-1, 3):
        assert lib(8, 8, 1, dt) == 0
    for lay in (-1, 2, 1 << 30):
        assert lib(8, 8, lay, 0) == 0
    assert lib(0, 0) == 0                               # the native grid needs a context
    assert L.vp8hip_residual_size(None, None) == 0
    assert P.residual_sizes(8, 8, "float32", "i420") == (64 + 2 * 16) * 4
    assert P.residual_sizes(8, 8, "int8") == 0 and P.residual_sizes(8, 8, layout="nope") == 0


def test_grid_maps():
    for d in range(1, 65):
        x = np.arange(d)
        assert np.array_equal(R.grid_map(d, d), x)       # at the display size the sample itself
        for dst in range(1, 65):
            m = R.grid_map(dst, d)
            assert m.min() >= 0 and m.max() < d, (dst, d)
            assert (np.diff(m) >= 0).all(), (dst, d)
    # the extremes stay inside, in the integers the kernel uses (below 2^31): luma and chroma
    for dst, d in ((16383, 16383), (1, 16383), (16383, 1), (16383, 16382), (8192, 8192), (8192, 1), (1, 8192)):
        m = R.grid_map(dst, d)
        assert m.min() >= 0 and m.max() < d and int((2 * (dst - 1) + 1) * d) < 2 ** 31

    class H:
        width, height, mb_cols, mb_rows = 131, 97, 9, 7
    for dw, dh in ((131, 97), (1, 1), (7, 3), (224, 224), (262, 194), (16383, 5)):
        gw, gh, cw, ch, sx, sy, scx, scy = R.grid(H, dw, dh)
        assert (gw, gh, cw, ch) == (dw, dh, (dw + 1) // 2, (dh + 1) // 2)
        assert len(sx) == gw and len(sy) == gh and len(scx) == cw and len(scy) == ch
        assert sx.max() < 131 and sy.max() < 97 and scx.max() < 66 and scy.max() < 49          # inside the display, so inside the coded area
        if (dw, dh) == (131, 97):                        # the display size: a crop, chroma under its luma
            assert np.array_equal(sx, np.arange(131)) and np.array_equal(scy, np.arange(49))
            assert np.array_equal(sx >> 1, scx.repeat(2)[:131])
    gw, gh, cw, ch, sx, sy, scx, scy = R.grid(H)
    assert (gw, gh, cw, ch) == (144, 112, 72, 56) and np.array_equal(sy, np.arange(112)) and np.array_equal(scx, np.arange(72))
