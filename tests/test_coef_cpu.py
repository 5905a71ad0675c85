"""CPU: tests/coef_reference.py -- the numpy restatement of vp8hip_frames_coef_async's definition (include/vp8hip.h) that the GPU tests
compare with bit for bit -- held against what is already pinned: the inverse DCT of its DEQUANT blocks is residual_reference.py's
residual for every sample, its Y2 path and its dequantiser are the oracle's int16 outputs, its LEVELS are the dense coefficients of
consistent IR.  Plus the library's host side through ctypes: vp8hip_dequant_factors, and vp8hip_coef_size, which has only the native
grid of a context and so, without a GPU, can be asked for its refusals alone (test_gpu_coef.py asks for the sizes)."""
import ctypes
import itertools

import numpy as np
import pytest

from vp8_testlib import ZIGZAG_RASTER, oracle, synth_ir
import coef_reference as C
import residual_reference as R

# the identity's inputs: (width, height, seeds), each seed also + 100 as an inter frame
IDENTITY = ((16, 16, (1, 2, 3, 4, 5, 6)), (67, 45, (7, 8)), (176, 144, (7, 8)))


def frames():
    for w, h, seeds in IDENTITY:
        for seed, inter in itertools.product(seeds, (False, True)):
            yield (w, h, seed, inter), synth_ir(w, h, seed + 100 * inter, inter=inter, big=True, segmented=True, dense=0.5)


def test_identity_with_the_residual():
    """the reference's inverse DCT of every DEQUANT block is the residual's block: no sample left out, lone DCs and empty blocks included"""
    samples = nonzero = 0
    for what, (hdr, mbs, coef, _) in frames():
        dq = C.coef_blocks(hdr, mbs, coef, "dequant")
        assert dq.min() >= -32768 and dq.max() <= 32767, what
        res = R.residual_blocks(hdr, mbs, coef)
        assert np.array_equal(R.idct(dq[:, :24]), res), what
        samples += res.size
        nonzero += int((res != 0).sum())
    assert samples == 179712 and nonzero * 3 > samples


def test_y2_gives_the_luma_dcs():
    """inv_walsh of the DEQUANT Y2 plane -- with eob <= 1 the _1 rule -- is luma position (0, 0) of a macroblock that has a Y2 block"""
    n = [0, 0]
    for what, (hdr, mbs, coef, _) in frames():
        dq = C.coef_blocks(hdr, mbs, coef, "dequant")
        kind, has_y2 = C.block_kinds(mbs)
        live = has_y2 & ((mbs[:, R.O_FLAGS] & R.MB_SKIP) == 0)
        eob24 = mbs[:, R.O_EOBS + 24]
        full = live & (eob24 > 1)
        assert np.array_equal(R.inv_walsh(dq[full, 24]).reshape(-1, 16), dq[full, :16, 0, 0]), what
        one = live & (eob24 <= 1)
        assert not dq[one, 24].reshape(-1, 16)[:, 1:].any()
        assert np.array_equal(np.repeat(R.s16((dq[one, 24, 0, 0] + 3) >> 3)[:, None], 16, 1), dq[one, :16, 0, 0]), what
        assert not dq[~has_y2, 24].any() and not dq[~live & has_y2].any()
        n[0] += int(full.sum())
        n[1] += int(one.sum())
    assert min(n) > 20, n


def _raster(block):
    return np.ascontiguousarray(np.asarray(block).reshape(4, 4).T).reshape(16)


def _extreme_headers():
    """synthetic frames at base_qindex 0 and 127 and with hand-set deltas of +-15"""
    for seed, qindex, delta in ((1, 0, -15), (2, 127, 15), (3, 0, 15), (4, 127, -15), (5, None, None), (6, 64, 15)):
        hdr, mbs, coef, _ = synth_ir(64, 48, seed, inter=seed % 2 == 1, big=True, dense=0.6)
        if qindex is not None:
            hdr.segmentation_enabled, hdr.base_qindex = int(seed > 4), qindex
            for f in ("y1dc_delta_q", "y2dc_delta_q", "y2ac_delta_q", "uvdc_delta_q", "uvac_delta_q"):
                setattr(hdr, f, delta)
        yield seed, hdr, mbs, coef


def test_against_the_oracle_bit_for_bit(pkg):
    """DEQUANT blocks against vp8o_dequantize_b, the Y2 path against vp8o_short_inv_walsh4x4 / _1, the factors -- the library's
    vp8hip_dequant_factors and the restatement's -- against vp8o_mb_dequant"""
    P = pkg
    O = oracle()
    vp = ctypes.c_void_p
    O.vp8o_dequantize_b.argtypes = [vp, vp, vp]
    O.vp8o_short_inv_walsh4x4.argtypes = [vp, vp]
    O.vp8o_short_inv_walsh4x4_1.argtypes = [vp, vp]
    O.vp8o_mb_dequant.argtypes = [vp, ctypes.c_int, vp]
    blocks = wrapped = 0
    n_y2 = [0, 0]
    for seed, hdr, mbs, coef in _extreme_headers():
        f = R.factors(hdr)
        got = P.dequant_factors(hdr)
        assert got.dtype == np.int16 and got.shape == (4, 6)
        for seg in range(4):
            dq6 = (ctypes.c_short * 6)()
            O.vp8o_mb_dequant(ctypes.byref(hdr), seg, dq6)
            assert list(dq6) == f[seg].tolist() == got[seg].tolist(), (seed, seg)
        lv = C.coef_blocks(hdr, mbs, coef, "levels")
        dq = C.coef_blocks(hdr, mbs, coef, "dequant")
        kind, has_y2 = C.block_kinds(mbs)
        for i in range(hdr.mb_rows * hdr.mb_cols):
            seg = int(mbs[i, R.O_SEGMENT]) & 3
            live = bool(has_y2[i]) and not mbs[i, R.O_FLAGS] & R.MB_SKIP
            for b in range(25):
                dcf, acf = (f[seg, 0], f[seg, 1]) if b < 16 else (f[seg, 4], f[seg, 5]) if b < 24 else (f[seg, 2], f[seg, 3])
                dqc = np.array([dcf] + [acf] * 15, np.int16)
                q = lv[i, b].reshape(16).astype(np.int16)
                out = np.zeros(16, np.int16)
                O.vp8o_dequantize_b(q.ctypes.data, dqc.ctypes.data, out.ctypes.data)
                want = dq[i, b].reshape(16).copy()
                if b < 16 and live:
                    want[0] = out[0]                                        # (the WHT's DC: below)
                assert np.array_equal(out, want), (seed, i, b)
                wrapped += int((out.astype(np.int64) != q.astype(np.int64) * dqc).sum())
                blocks += 1
            if live:
                y2 = dq[i, 24].reshape(16).astype(np.int16)
                dcs = np.zeros(256, np.int16)
                if mbs[i, R.O_EOBS + 24] > 1:
                    O.vp8o_short_inv_walsh4x4(y2.ctypes.data, dcs.ctypes.data)
                else:
                    O.vp8o_short_inv_walsh4x4_1(y2.ctypes.data, dcs.ctypes.data)
                assert np.array_equal(dcs[::16], dq[i, :16, 0, 0]), (seed, i)
                n_y2[int(mbs[i, R.O_EOBS + 24] > 1)] += 1
    assert blocks > 1000 and wrapped > 0 and min(n_y2) > 0
    with pytest.raises((ValueError, TypeError, ctypes.ArgumentError)):
        P.dequant_factors(None)
    assert P.load_hip().vp8hip_dequant_factors(None, None) == -2


def test_levels_consistency():
    """LEVELS is the dense coefficients of consistent IR outside skipped macroblocks; re-dequantised it is DEQUANT outside the luma DCs
    that come out of a Y2 block"""
    for what, (hdr, mbs, coef, _) in frames():
        lv = C.coef_blocks(hdr, mbs, coef, "levels")
        dq = C.coef_blocks(hdr, mbs, coef, "dequant")
        dense = np.asarray(coef, np.int64).reshape(-1, 25, 4, 4).transpose(0, 1, 3, 2)
        live = (mbs[:, R.O_FLAGS] & R.MB_SKIP) == 0
        assert np.array_equal(lv[live], dense[live]), what
        assert not lv[~live].any()
        f = R.factors(hdr)[mbs[:, R.O_SEGMENT] & 3]
        fac = np.empty(lv.shape, np.int64)
        for blocks, dc, ac in ((slice(0, 16), 0, 1), (slice(16, 24), 4, 5), (slice(24, 25), 2, 3)):
            fac[:, blocks] = f[:, ac][:, None, None, None]
            fac[:, blocks, 0, 0] = f[:, dc][:, None]
        again = R.s16(lv * fac)
        _, has_y2 = C.block_kinds(mbs)
        keep = np.ones(lv.shape, bool)
        keep[has_y2, :16, 0, 0] = False
        assert np.array_equal(again[keep], dq[keep]), what


def test_arrange_and_sizes():
    """the tensor of the restatement: the planes back to back, channel j of "raster" position j, of "zigzag" the scan's, "inplace" the
    residual's geometry"""
    hdr, mbs, coef, _ = synth_ir(67, 45, 9, big=True, dense=0.5)
    blocks = C.coef_blocks(hdr, mbs, coef, "levels")
    rows, cols = hdr.mb_rows, hdr.mb_cols
    views, flat = C.arrange(blocks, hdr, "inplace", C.PLANES)
    assert [v.shape for v in views.values()] == [(16 * rows, 16 * cols), (8 * rows, 8 * cols), (8 * rows, 8 * cols), (4 * rows, 4 * cols)]
    assert flat.nbytes == C.size(hdr, "inplace", C.PLANES) == 400 * rows * cols * 2
    mb, b, v, u = 2 * cols + 3, 6, 2, 1                                  # luma block (1, 2) of macroblock (2, 3)
    assert views["y"][16 * 2 + 4 * 1 + v, 16 * 3 + 4 * 2 + u] == blocks[mb, b, v, u] == coef[mb, b * 16 + u * 4 + v]
    assert views["v"][8 * 2 + 4 * 1 + v, 8 * 3 + u] == blocks[mb, 22, v, u]
    for order, nfreq in itertools.product(("raster", "zigzag"), (1, 3, 10, 16)):
        ch, flat = C.arrange(blocks, hdr, "channels", ("u", "y2", "y"), nfreq, order)
        assert list(ch) == ["y", "u", "y2"] and ch["y"].shape == (nfreq, 4 * rows, 4 * cols) and ch["y2"].shape == (nfreq, rows, cols)
        assert flat.nbytes == C.size(hdr, "channels", ("y", "u", "y2"), nfreq) == nfreq * 21 * rows * cols * 2
        for j in range(nfreq):
            p = C.ZIGZAG[j] if order == "zigzag" else j
            assert ch["y"][j, 4 * 2 + 1, 4 * 3 + 2] == blocks[mb, b, p >> 2, p & 3]
            assert ch["y2"][j, 2, 3] == blocks[mb, 24, p >> 2, p & 3]


def test_zigzag(pkg):
    """a permutation, and the reference's scan: the one the synthetic IR is made with and the one the package states"""
    assert sorted(C.ZIGZAG) == list(range(16))
    assert list(C.ZIGZAG) == list(ZIGZAG_RASTER) == list(pkg.COEF_ZIGZAG)
    # as the stream walks it: position after position of the scan, eob the first one not coded
    hdr, mbs, coef, _ = synth_ir(64, 48, 12, big=True, dense=0.8)
    lv = C.coef_blocks(hdr, mbs, coef, "levels").reshape(-1, 25, 16)[:, :, list(C.ZIGZAG)]
    kind, _ = C.block_kinds(mbs)
    eobs = mbs[:, R.O_EOBS:R.O_EOBS + 25]
    checked = 0
    for i, b in zip(*np.nonzero(kind == 2)):
        if eobs[i, b] < 15:                          # (synth_ir writes 15 for a block coded to its last position, too)
            assert not lv[i, b, eobs[i, b]:].any() and lv[i, b, eobs[i, b] - 1] != 0
            checked += 1
    assert checked > 100


def test_size_function_of_the_library(pkg):
    """without a context vp8hip_coef_size is 0 for everything -- there is only a context's native grid -- and the wrapper's coef_size
    with it; the parameters it refuses are the call's (test_gpu_coef.py: the sizes on a context, and the refusals again)"""
    P = pkg
    L = P.load_hip()
    for stage, layout, order, nfreq, planes, dtype in itertools.product((0, 1), (0, 1), (0, 1), range(1, 17), range(1, 16), (0, 1, 2)):
        p = P.CoefParams(stage, layout, order, nfreq, planes, dtype)
        assert L.vp8hip_coef_size(None, ctypes.byref(p)) == 0
    for bad in (P.CoefParams(2, 0, 0, 16, 7, 0), P.CoefParams(0, 2, 0, 16, 7, 0), P.CoefParams(0, 0, 2, 16, 7, 0), P.CoefParams(0, 0, 0, 0, 7, 0),
                P.CoefParams(0, 0, 0, 17, 7, 0), P.CoefParams(0, 0, 0, 16, 0, 0), P.CoefParams(0, 0, 0, 16, 16, 0), P.CoefParams(0, 0, 0, 16, 7, 3),
                P.CoefParams(0, 1, 0, 15, 7, 0), P.CoefParams(0, 1, 1, 16, 7, 0), P.CoefParams(-1, 0, 0, 16, 7, -1)):
        assert L.vp8hip_coef_size(None, ctypes.byref(bad)) == 0
    assert L.vp8hip_coef_size(None, None) == 0
    assert P.coef_size(None) == 0 and P.coef_size(None, "levels", "inplace", ("y", "y2")) == 0
    assert P.coef_size(None, stage="nope") == 0 and P.coef_size(None, planes=("w",)) == 0 and P.coef_size(None, dtype="int8") == 0
    assert ctypes.sizeof(P.CoefParams) == 40
    # what the restatement says of sizes, by hand: 130x98 is 9 x 7 macroblocks
    hdr = P.FrameHdr()
    hdr.width, hdr.height, hdr.mb_cols, hdr.mb_rows = 130, 98, 9, 7
    assert C.size(hdr) == 16 * (16 + 4 + 4) * 63 * 2 and C.size(hdr, "channels", ("y2",), 3, "f32") == 3 * 63 * 4
    assert C.size(hdr, "inplace", ("u", "y2"), 16, "f16") == (64 + 16) * 63 * 2
    # split_coef, the wrapper's views, on numpy: the restatement's
    hdr2, mbs, coef, _ = synth_ir(130, 98, 5, big=True, dense=0.5)
    blocks = C.coef_blocks(hdr2, mbs, coef, "dequant")
    for layout, nfreq, planes in (("channels", 5, ("y", "v", "y2")), ("inplace", 16, ("u", "y2")), ("channels", 16, C.PLANES)):
        views, flat = C.arrange(blocks, hdr2, layout, planes, nfreq)
        got = P.split_coef(flat[None], 9, 7, layout, planes, nfreq)
        assert list(got) == list(views)
        for name in views:
            assert np.array_equal(got[name][0], views[name]), (layout, name)
    with pytest.raises(ValueError):
        P.split_coef(np.zeros((1, 10), np.int16), 9, 7)
