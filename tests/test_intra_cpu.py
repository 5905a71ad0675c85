"""CPU: the restatement of vp8hip_frames_intra_async (tests/intra_reference.py) and the two host helpers vp8hip_intra_costs and
vp8hip_intra_rd against the REFERENCE: tests/golden/intra_ref.json holds what the reference's own key-frame macroblock loop makes of
the cases' pictures (recorded by tests/golden/make_intra_fixtures.py through intra_ref_driver.c), intra_ref_md5.json what the
reference decoder makes of the key frames written from the restatement's modes and levels.  error16x16 and error4x4 are locals of
the reference's picker: the driver makes both a second time from the reference's own functions, and the picker's decision and rate
hold the driver's figures in turn."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import intra_reference as IR
import quant_reference as QR
from residual_reference import idct
from vp8_testlib import ROOT
from vp8_writer import write_ivf

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_intra_fixtures as MF  # noqa: E402

with open(os.path.join(HERE, "golden", "intra_ref.json")) as _f:
    FIXTURE = json.load(_f)
with open(os.path.join(HERE, "golden", "intra_ref_md5.json")) as _f:
    MD5 = json.load(_f)
REF_MD5 = os.path.join(ROOT, "oracle", "_ref", "ref_md5")


@pytest.fixture(scope="module")
def costs(pkg):
    H = pkg.load_host()
    return IR.intra_costs(list((ctypes.c_uint16 * 256).in_dll(H, "vp8t_prob_cost")), list((ctypes.c_uint8 * 900).in_dll(H, "vp8t_kf_bmode_probs")))


@pytest.fixture(scope="module")
def restated(costs):
    """the restatement of every fixture case with the reference's loop bound, computed once"""
    out = {}
    for c in MF.CASES:
        display, kind, seed, q, deltas, quantizer, zbin = c
        rec = FIXTURE["cases"][MF.case_key(c)]
        src = IR.picture(kind, *MF.aligned(display), seed)
        out[MF.case_key(c)] = IR.intra_planes(src, q, deltas, quantizer, zbin, rec["rdmult"], rec["rddiv"], costs[0], costs[1], 3)
    return out


def test_the_helpers_are_the_references(pkg, costs):
    """vp8hip_intra_costs is vp8_init_mode_costs' key-frame part, vp8hip_intra_rd vp8_initialize_rd_consts for all 128 qindex values;
    the restatement's helpers agree"""
    h = FIXTURE["helpers"]
    mb, b = pkg.intra_costs()
    assert mb.tolist() == h["mbmode_cost"] and b.ravel().tolist() == h["bmode_cost"]
    assert costs[0].tolist() == h["mbmode_cost"] and costs[1].ravel().tolist() == h["bmode_cost"]
    assert max(h["bmode_cost"]) <= 65535 and min(h["bmode_cost"]) >= 0
    for q in range(128):
        assert list(pkg.intra_rd(q)) == h["rd"][q] == list(IR.intra_rd(q)), q
        assert 0 <= h["rd"][q][0] <= 1000 and h["rd"][q][1] in (1, 100)
    for c in MF.CASES:                                               # the y1dc delta and the zbin_over_quant branch
        rec = FIXTURE["cases"][MF.case_key(c)]
        assert pkg.intra_rd(c[3], c[4][0], c[6][0]) == (rec["rdmult"], rec["rddiv"]) == IR.intra_rd(c[3], c[4][0], c[6][0]), c
    assert any(c[6][0] > 0 and pkg.intra_rd(c[3], c[4][0], c[6][0]) != pkg.intra_rd(c[3], c[4][0], 0) for c in MF.CASES)
    rdmult, rddiv = ctypes.c_int(), ctypes.c_int()
    L = pkg.load_hip()
    for bad in ((-1, 0), (128, 0), (40, 16), (40, -16)):
        assert L.vp8hip_intra_rd(bad[0], bad[1], 0, ctypes.byref(rdmult), ctypes.byref(rddiv)) == -2
    assert L.vp8hip_intra_rd(40, 0, 0, None, ctypes.byref(rddiv)) == -2 and L.vp8hip_intra_costs(None) == -2
    assert pkg.intra_sizes(67, 45, ("rd16", "eobs")) == (800 * 15, 32 * 15, 4 * 2 * 15, 67 * 45 + 2 * 34 * 23, 32 * 15)
    assert pkg.intra_sizes(0, 45) == (0, 0, 0, 0, 0) and pkg.intra_sizes(16, 16, ("erry",)) == (0, 0, 0, 0, 0)


@pytest.mark.parametrize("case", MF.CASES, ids=MF.case_key)
def test_restatement_is_the_reference(restated, case):
    """modes, levels, eobs, the three figures, the skip flag and the reconstruction of every case, as the reference's own loop gives
    them"""
    rec, o = FIXTURE["cases"][MF.case_key(case)], restated[MF.case_key(case)]
    n = o["modes"].shape[0] * o["modes"].shape[1]
    m = o["modes"].reshape(n, 32)
    bp = m[:, 0] == IR.B_PRED
    modes = np.full((n, 18), 255, np.uint8)
    modes[:, 0], modes[:, 1] = m[:, 0], m[:, 1]
    modes[bp, 2:] = m[bp, 4:20]
    assert MF.same(rec["modes"], modes)
    assert all((m[i, 4:20] == IR.IMPLIED_BMODE[int(m[i, 0])]).all() for i in np.flatnonzero(~bp))
    assert not m[:, 3].any() and not m[:, 20:].any()
    assert MF.same(rec["levels"], o["levels"].reshape(n, 25, 16))
    assert MF.same(rec["eob"], o["eob"].reshape(n, 32)[:, :25]) and not o["eob"][..., 25:].any()
    assert MF.same(rec["rate"], o["stats"]["rate"].astype(np.int32))
    assert MF.same(rec["skip"], m[:, 2])
    assert MF.same(rec["rd16"], o["stats"]["rd16"].astype(np.int32))
    assert MF.same(rec["rd4"], o["stats"]["rd4"].astype(np.int32))
    assert MF.same(rec["rec"], np.concatenate([p.ravel() for p in o["rec"]]))
    assert (o["stats"]["eobs"].ravel() == o["eob"].reshape(n, 32).sum(axis=1)).all()
    assert ((o["stats"]["rd4"] < o["stats"]["rd16"]).ravel() == bp).all()


def test_the_cases_leave_no_path_untested(restated):
    """each y mode, each uv mode, each sub-block mode tried and chosen, a break-out, B_PRED blocks with eob <= 1 and above, Y2 blocks with
    eob <= 1 and above, a skippable macroblock, a last-column macroblock in a row > 0 that chose B_PRED"""
    ymodes, uvmodes, tried, chosen, seen = set(), set(), set(), set(), {}
    for o in restated.values():
        ymodes |= set(o["modes"][..., 0].ravel().tolist())
        uvmodes |= set(o["modes"][..., 1].ravel().tolist())
        tried |= o["seen"]["tried"]
        chosen |= o["seen"]["bmodes"]
        for k, v in o["seen"].items():
            if isinstance(v, int):
                seen[k] = seen.get(k, 0) + v
    assert ymodes == {0, 1, 2, 3, 4} and uvmodes == {0, 1, 2, 3} and tried == {0, 1, 2, 3}
    assert chosen == {IR.B_DC, IR.B_TM, IR.B_VE, IR.B_HE}                # ... and each of the four is chosen by some B_PRED macroblock
    for k in ("breakout", "bpred_eob_le1", "bpred_eob_gt1", "y2_eob_le1", "y2_eob_gt1", "skippable", "last_col_bpred"):
        assert seen[k] > 0, k


def test_one_block_forms_agree_with_the_array_forms():
    """the sub-block chain's plain-integer fdct, quantiser and idct against quant_reference's and residual_reference's"""
    rng = np.random.default_rng(4)
    for q, deltas, zbin in ((0, (0, 0, 0, 0, 0), (0, 0, 0)), (40, (3, -2, 5, -4, 7), (20, 3, -2)), (127, (0, 0, 0, 0, 0), (0, 0, 0))):
        f = QR.quant_factors(q, deltas)
        extra = QR.zbin_extra(f, *zbin)
        for amp in (2, 40, 255):
            d = rng.integers(-amp, amp + 1, (4, 4))
            c = IR.fdct4([int(v) for v in d.ravel()])
            assert c == QR.fdct(d[None])[0].ravel().tolist()
            coef = np.zeros((1, 25, 16), np.int64)
            coef[0, 0] = c
            for quantizer in QR.QUANTIZERS:
                lv, dq, eob = IR.quant4(c, f, extra, QR.Y1, quantizer)
                a, b, e = QR.quantise(coef, f, extra, quantizer)
                assert lv == a[0, 0].tolist() and dq == b[0, 0].tolist() and eob == int(e[0, 0])
                assert IR.idct4(dq) == idct(np.array(dq).reshape(1, 4, 4), QR.fit)[0].ravel().tolist()


@pytest.mark.parametrize("last", [3, 9])
@pytest.mark.parametrize("closure", MF.CLOSURE, ids=lambda c: f"{c[0][0]}x{c[0][1]}")
def test_closure_through_the_writer_and_the_reference_decoder(costs, closure, last, tmp_path):
    """the restatement's modes and transposed levels as an IR through vp8_writer.write_key_frame with filter level 0: the reference
    decoder's picture is the restatement's rec (its MD5 recorded for machines where the reference is not built)"""
    display, kind, seed, q = closure
    o, data = MF.closure_stream(display, kind, seed, q, last, costs)
    rec = MD5[f"{display[0]}x{display[1]}_last{last}"]
    assert hashlib.sha256(data).hexdigest() == rec["stream_sha256"]
    mine = hashlib.md5(IR.rec_i420(o, *display).tobytes()).hexdigest()
    assert mine == rec["md5"]
    if os.path.exists(REF_MD5):
        ivf, out = tmp_path / "s.ivf", tmp_path / "s.md5"
        write_ivf(ivf, display[0], display[1], [data])
        r = subprocess.run([REF_MD5, str(ivf), str(out)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert open(out).read().split()[0] == mine
    chosen = set(o["modes"][o["modes"][..., 0] == IR.B_PRED][:, 4:20].ravel().tolist())
    assert chosen <= set(range(last + 1)) and (last == 3 or chosen == set(range(10)))
