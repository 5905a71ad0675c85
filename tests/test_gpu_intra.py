"""GPU (-m gpu): intra modes and levels of key-frame macroblocks in device memory (vp8hip_frames_intra_async; Vp8Hip.frames_intra;
csrc/hip/vp8_intra_enc.hip), byte for byte against the restatement (tests/intra_reference.py, itself held to the reference by
tests/test_intra_cpu.py) applied to the coded planes: level records, eobs, the five planes, the reconstruction and the modes.  The
closure test makes the first stream whose every frame was encoded on the device.  torch is imported here, before the package loads
libvpx's library: one HIP runtime per process."""
import ctypes
import hashlib
import json
import os

import torch  # noqa: F401  (first: the library then shares torch's HIP runtime)
import numpy as np
import pytest

from handover_testlib import assert_destinations_refused, assert_guards_intact, guarded, large_launch, picture_into
import intra_reference as IR
import scale_reference as SC
import tfilter_reference as TR
from vp8_testlib import synth_ir
from vp8_writer import write_key_frame

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
OUTPUTS = ("coef", "eob", "stats", "rec", "modes")
ALL_PLANES = tuple(IR.STATS)


def coded(ctx, fb):
    return [np.ascontiguousarray(p) for p in SC.planes(ctx.download_full(fb), ctx.g)]


def upload(ctx, fb, planes, rng):
    """a picture's three coded planes inside a frame buffer image of other bytes: the raster borders hold garbage"""
    ctx.upload_frame(fb, picture_into(rng.integers(0, 256, ctx.g.frame_size, dtype=np.uint8), ctx.g, planes))


@pytest.fixture(scope="module")
def costs(pkg):
    return pkg.intra_costs()


def restate(costs, src, q=40, deltas=(0, 0, 0, 0, 0), quantizer="regular", zbin=(0, 0, 0), bmode_last=3, bpred=True, rd=None):
    rdm, rdd = rd or IR.intra_rd(q, deltas[0], zbin[0])
    return IR.intra_planes(src, q, deltas, quantizer, zbin, rdm, rdd, costs[0], costs[1], bmode_last, 0 if bpred else IR.NO_BPRED)


def expected(o, display, stage="levels", planes=ALL_PLANES):
    out = {"coef": o[stage], "eob": o["eob"], "rec": IR.rec_i420(o, *display), "modes": o["modes"]}
    if planes:
        out["stats"] = IR.stats_tensor(o, planes)
    return out


def host(got):
    return {k: t.cpu().numpy().view(np.uint32) if k == "stats" else t.cpu().numpy() for k, t in got.items()}


def compare(got, want, i, what):
    for k, t in got.items():
        a = t[i] if isinstance(t, np.ndarray) else host({k: t[i:i + 1]})[k][0]
        bad = np.flatnonzero(a.ravel() != want[k].ravel())
        assert not bad.size, (what, i, k, bad[:8].tolist(), a.ravel()[bad[:8]].tolist(), want[k].ravel()[bad[:8]].tolist())


@pytest.fixture(scope="module")
def contexts(pkg):
    made = {}

    def get(size, fbs=4):
        if (size, fbs) not in made:
            ctx = pkg.Vp8Hip(0)
            ctx.configure(size[0], size[1], fbs, 1)
            made[(size, fbs)] = ctx
        return made[(size, fbs)]
    yield get
    for ctx in made.values():
        ctx.close()


def aligned(display):
    return (display[0] + 15) // 16 * 16, (display[1] + 15) // 16 * 16


# display, content, seed, qindex, deltas, quantizer, zbin, bmode_last, bpred
CASES = [
    ((16, 16), "decoded", 1, 40, (0, 0, 0, 0, 0), "regular", (0, 0, 0), 3, True),
    ((32, 32), "noise", 2, 10, (0, 0, 0, 0, 0), "regular", (0, 0, 0), 9, True),
    ((48, 32), "decoded", 3, 40, (0, 0, 0, 0, 0), "fast", (0, 0, 0), 3, True),
    ((48, 32), "gradient", 4, 3, (0, 1, 0, 0, 0), "regular", (0, 0, 0), 9, True),
    ((48, 32), "flat", 0, 127, (0, 0, 0, 0, 0), "regular", (0, 0, 0), 3, True),
    ((67, 45), "decoded", 5, 40, (3, -2, 5, -4, 7), "regular", (20, 0, 0), 3, True),
    ((67, 45), "noise", 6, 112, (0, 0, 0, 0, 0), "regular", (0, 9, 5), 9, True),
    ((67, 45), "gradient", 7, 0, (0, 0, 0, 0, 0), "fast", (0, 0, 0), 3, False),
    ((48, 32), "vstripes", 22, 10, (0, 0, 0, 0, 0), "regular", (0, 0, 0), 3, True),
    ((48, 32), "hstripes", 23, 10, (0, 0, 0, 0, 0), "fast", (0, 0, 0), 9, True),
    ((176, 144), "decoded", 8, 40, (0, 0, 0, 0, 0), "regular", (0, 0, 0), 3, True),
    ((176, 144), "gradient", 9, 60, (-15, 15, -15, 15, -15), "regular", (0, 0, 0), 9, True),
]


def case_id(c):
    return f"{c[0][0]}x{c[0][1]}_{c[1]}_q{c[3]}_{c[5]}_last{c[7]}" + ("" if c[8] else "_nobpred")


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_cases_from_raster(pkg, contexts, costs, case):
    """sizes, contents and settings from uploaded frame buffers with garbage in their borders: all five outputs, both stages"""
    display, kind, seed, q, deltas, quantizer, zbin, last, bpred = case
    ctx = contexts(display)
    src = IR.picture(kind, *aligned(display), seed)
    upload(ctx, 0, src, np.random.default_rng(seed))
    o = restate(costs, src, q, deltas, quantizer, zbin, last, bpred)
    rd = IR.intra_rd(q, deltas[0], zbin[0])
    assert pkg.intra_rd(q, deltas[0], zbin[0]) == rd
    for stage in ("levels", "dequant"):
        got = ctx.frames_intra([0], q, deltas, quantizer, stage, zbin, bmode_last=last, bpred=bpred, planes=ALL_PLANES, want=OUTPUTS)
        assert set(got) == set(OUTPUTS)
        compare(got, expected(o, display, stage), 0, (case_id(case), stage))


@pytest.mark.parametrize("display", [(16, 1136), (48, 1136), (2064, 16)], ids=["one_column_71_rows", "three_columns_71_rows", "one_row_129_columns"])
def test_tall_and_wide(pkg, contexts, costs, display):
    """more rows than a workgroup has waves and than a band has rows -- with one column, and with three, where the first row of the
    second band reads its above-left and above-right neighbours from the line the first band left --; a single row of 129 macroblocks"""
    ctx = contexts(display)
    src = IR.picture("decoded", *display, 12)
    upload(ctx, 1, src, np.random.default_rng(12))
    for last in (3, 9):
        o = restate(costs, src, 30, bmode_last=last)
        got = ctx.frames_intra([1], 30, bmode_last=last, planes=ALL_PLANES, want=OUTPUTS)
        compare(got, expected(o, display), 0, (display, last))


def test_1080p_against_recorded_digests(pkg, contexts):
    """1920x1080 once: SHA-256 of each output against those recorded from the restatement (tests/golden/make_intra_fixtures.py)"""
    with open(os.path.join(HERE, "golden", "intra_1080p_sha256.json")) as f:
        rec = json.load(f)
    ctx = contexts((1920, 1080), 1)
    src = IR.picture(rec["content"], 1920, 1088, rec["seed"])
    upload(ctx, 0, src, np.random.default_rng(1))
    got = host(ctx.frames_intra([0], rec["qindex"], bmode_last=rec["bmode_last"], planes=ALL_PLANES, want=OUTPUTS))
    for k in OUTPUTS:
        assert hashlib.sha256(np.ascontiguousarray(got[k][0]).tobytes()).hexdigest() == rec["sha256"][k], k


def test_job_qindex_and_each_output_alone(pkg, contexts, costs):
    """ten qindex values in one call (more than a launch has tables); each output alone and in pairs gives the same bytes; twice"""
    ctx = contexts((48, 32))
    rng = np.random.default_rng(3)
    pics = [IR.picture("decoded", 48, 32, 31), IR.picture("noise", 48, 32, 32), IR.picture("gradient", 48, 32, 33)]
    for fb, p in enumerate(pics):
        upload(ctx, fb, p, rng)
    qs = [0, 3, 17, 40, 40, 63, 90, 112, 127, 5, 77, 101]
    fbs = [i % 3 for i in range(len(qs))]
    assert len(set(qs)) > 10
    rd = (300, 1)
    kw = dict(rdmult=rd[0], rddiv=rd[1], bmode_last=9)
    full = ctx.frames_intra(fbs, qs, planes=ALL_PLANES, want=OUTPUTS, **kw)
    again = ctx.frames_intra(fbs, qs, planes=ALL_PLANES, want=OUTPUTS, **kw)
    for i, (fb, q) in enumerate(zip(fbs, qs)):
        compare(host(full), expected(restate(costs, pics[fb], q, bmode_last=9, rd=rd), (48, 32)), i, ("job_qindex", q))
    assert all(torch.equal(full[k], again[k]) for k in OUTPUTS)
    for want in (("coef",), ("eob",), ("rec",), ("modes",), ("coef", "modes"), ("eob", "rec")):
        got = ctx.frames_intra(fbs, qs, want=want, **kw)
        assert set(got) == set(want) and all(torch.equal(got[k], full[k]) for k in want), want
    for planes in (("rd16",), ("recsse",), ("eobs", "rd4"), ("rate", "rd16", "eobs")):
        got = ctx.frames_intra(fbs, qs, planes=planes, want=(), **kw)
        assert set(got) == {"stats"}
        bits = [list(IR.STATS).index(p) for p in sorted(planes, key=list(IR.STATS).index)]
        assert torch.equal(got["stats"], full["stats"][:, bits]), planes
    nob = ctx.frames_intra(fbs[:3], 40, bpred=False, planes=ALL_PLANES, want=OUTPUTS)
    for i in range(3):
        o = restate(costs, pics[i], 40, bpred=False)
        assert (o["stats"]["rd4"] == IR.INT_MAX).all() and (o["modes"][..., 0] < 4).all()
        compare(nob, expected(o, (48, 32)), i, "no_bpred")


def raw_call(ctx, P, costs, fbs, q=40, deltas=(0, 0, 0, 0, 0), quantizer=0, stage=1, zbin=(0, 0, 0), jq=None, rdmult=300, rddiv=1, last=3, flags=0, planes=0,
             mb=None, bc=None, coef=None, coef_stride=0, eob=None, eob_stride=0, stats=None, stats_stride=0, rec=None, rec_stride=0, modes=None,
             modes_stride=0, n=None):
    """vp8hip_frames_intra_async itself, on pointers: -> its status"""
    vp = ctypes.c_void_p
    keep = None if jq is None else (ctypes.c_uint8 * len(jq))(*jq)
    p = P.IntraParams()
    p.q = P.QuantParams(q, (ctypes.c_int * 5)(*deltas), quantizer, 0, stage, zbin[0], zbin[1], zbin[2], 0, keep)
    p.rdmult, p.rddiv, p.bmode_last, p.flags, p.planes = rdmult, rddiv, last, flags, planes
    p.cost.mbmode_cost[:] = [int(v) for v in (costs[0] if mb is None else mb)]
    flat = [int(v) for v in np.asarray(costs[1] if bc is None else bc).ravel()]
    ctypes.memmove(p.cost.bmode_cost, (ctypes.c_int * 1000)(*flat), 4000)
    arr = (ctypes.c_int * max(len(fbs), 1))(*fbs)
    return ctx.L.vp8hip_frames_intra_async(ctx.h, arr, len(fbs) if n is None else n, ctypes.byref(p), vp(coef) if coef else None, coef_stride,
                                           vp(eob) if eob else None, eob_stride, vp(stats) if stats else None, stats_stride, vp(rec) if rec else None,
                                           rec_stride, vp(modes) if modes else None, modes_stride)


def test_strides_and_alignment(pkg, contexts, costs):
    """every output with bytes between the jobs and at the least alignment it allows: the values, and the bytes around them"""
    display = (67, 45)
    ctx = contexts(display)
    rng = np.random.default_rng(11)
    pics = [IR.picture("decoded", 80, 48, 41), IR.picture("noise", 80, 48, 42)]
    for fb, p in enumerate(pics):
        upload(ctx, fb, p, rng)
    fbs = [0, 1, 0]
    wants = [expected(restate(costs, pics[fb], 40, rd=(300, 1)), display) for fb in fbs]
    csize, esize, ssize, rsize, msize = pkg.intra_sizes(67, 45, ALL_PLANES)
    assert (csize, esize, ssize, msize) == (800 * 15, 32 * 15, 4 * 5 * 15, 32 * 15)
    for (coff, cpad), (eoff, epad), (soff, spad), (roff, rpad), (moff, mpad) in (((16, 0), (4, 0), (4, 0), (1, 0), (4, 0)),
                                                                                  ((48, 16), (12, 4), (8, 12), (3, 5), (4, 8)),
                                                                                  ((0, 160), (0, 32), (0, 4), (7, 1), (12, 4))):
        cbig, cflat = guarded(3, csize, cpad, coff)
        ebig, eflat = guarded(3, esize, epad, eoff)
        sbig, sflat = guarded(3, ssize, spad, soff)
        rbig, rflat = guarded(3, rsize, rpad, roff)
        mbig, mflat = guarded(3, msize, mpad, moff)
        torch.cuda.synchronize()
        assert raw_call(ctx, pkg, costs, fbs, planes=31, coef=cflat.data_ptr(), coef_stride=csize + cpad, eob=eflat.data_ptr(), eob_stride=esize + epad,
                        stats=sflat.data_ptr(), stats_stride=ssize + spad, rec=rflat.data_ptr(), rec_stride=rsize + rpad, modes=mflat.data_ptr(),
                        modes_stride=msize + mpad) == 0
        ctx.sync()
        for i in range(3):
            got = {"coef": cflat.cpu().numpy()[i].view(np.int16), "eob": eflat.cpu().numpy()[i], "stats": sflat.cpu().numpy()[i].view(np.uint32),
                   "rec": rflat.cpu().numpy()[i], "modes": mflat.cpu().numpy()[i]}
            for k, a in got.items():
                assert np.array_equal(a.ravel(), wants[i][k].ravel()), (k, i, coff, cpad)
        for big, size, pad, off, what in ((cbig, csize, cpad, coff, "coef"), (ebig, esize, epad, eoff, "eob"), (sbig, ssize, spad, soff, "stats"),
                                          (rbig, rsize, rpad, roff, "rec"), (mbig, msize, mpad, moff, "modes")):
            assert_guards_intact(big, 3, size, pad, off, what=what)


def test_many_jobs(pkg, contexts, costs):
    """130 jobs of different content in one call; more jobs than a launch carries (256), repeats in any order; two calls back to back
    without a sync between them"""
    ctx = contexts((32, 32), 130)
    rng = np.random.default_rng(8)
    pics = [IR.picture(IR.CONTENTS[i % 4] if i % 4 != 2 else "noise", 32, 32, 100 + i) for i in range(130)]
    for fb, p in enumerate(pics):
        upload(ctx, fb, p, rng)
    rd = (200, 1)
    wants = [expected(restate(costs, p, 40, bmode_last=9, rd=rd), (32, 32)) for p in pics]
    assert len({w["coef"].tobytes() for w in wants}) > 100
    first = ctx.frames_intra(list(range(130)), 40, rdmult=rd[0], rddiv=rd[1], bmode_last=9, planes=ALL_PLANES, want=OUTPUTS)
    order = [int(k) for k in rng.integers(0, 130, 300)]
    second = ctx.frames_intra(order, 40, rdmult=rd[0], rddiv=rd[1], bmode_last=9, planes=ALL_PLANES, want=OUTPUTS)      # (no sync in between)
    first, second = host(first), host(second)
    for i in range(130):
        compare(first, wants[i], i, "130 jobs")
    for i, fb in enumerate(order):
        compare(second, wants[fb], i, "300 jobs")


@pytest.mark.parametrize("name", ["kf_odd_67x45", "kf_q0_176x144"])
def test_jobs_from_tiles(pkg, costs, name, monkeypatch):
    """frames a large launch left as tiles, mixed with an uploaded raster frame and a frame buffer never written; the context's
    memory does not change.  Expected values from pictures downloaded AFTER the calls: a download gives a tiled frame its raster form"""
    P = pkg
    n = 3
    ctx = P.Vp8Hip(0)
    try:
        large_launch(P, ctx, name, n, monkeypatch)
        ctx.sync()
        assert ctx.memory_usage()["raster_pool"] == 0 and ctx.memory_usage()["tile_pool"] > 0
        ctx.upload_frame(n, np.random.default_rng(67).integers(0, 256, ctx.g.frame_size, dtype=np.uint8))     # raster only
        before = ctx.memory_usage()
        fbs = [0, n, 1, n + 1, 2]
        first = ctx.frames_intra(fbs, 40, bmode_last=9, planes=ALL_PLANES, want=OUTPUTS)
        ctx.sync()
        assert ctx.memory_usage() == before
        pics = {k: coded(ctx, k) for k in range(n + 1)}
        pics[n + 1] = [np.zeros((ctx.g.aligned_h >> s, ctx.g.aligned_w >> s), np.uint8) for s in (0, 1, 1)]
        display = (ctx.width, ctx.height)
        for i, fb in enumerate(fbs):
            compare(first, expected(restate(costs, pics[fb], 40, bmode_last=9), display), i, (name, "tiles", fb))
        after = ctx.frames_intra(fbs, 40, bmode_last=9, planes=ALL_PLANES, want=OUTPUTS)                        # ... every frame in raster form
        assert all(torch.equal(after[k], first[k]) for k in OUTPUTS)
    finally:
        ctx.close()


def test_closure_first_stream_encoded_on_the_device(pkg, costs):
    """frames_intra -> write_key_frame (host, filter level 0) -> the product's decoder equals rec byte for byte; then frames_motion,
    frames_subpel, frames_quant and frames_pack of a second picture against that decoded key frame decode to frames_quant's rec"""
    P = pkg
    w, h, q = 48, 32, 40
    rows, cols = 2, 3
    ctx = P.Vp8Hip(0)
    parser = P.Parser()
    try:
        ctx.configure(w, h, 6, 1)
        first = IR.picture("decoded", w, h, 61)
        upload(ctx, 4, first, np.random.default_rng(2))
        got = ctx.frames_intra([4], q, bmode_last=9, want=("coef", "modes", "rec"))
        modes, levels = got["modes"][0].cpu().numpy(), got["coef"][0].cpu().numpy()
        assert (modes[..., 0] == 4).any() and levels.any()
        hdr_k, _, _, _ = synth_ir(w, h, 21, inter=False, segmented=False)
        hdr_k.filter_level, hdr_k.base_qindex, hdr_k.mode_ref_lf_delta_enabled = 0, q, 0
        for f in ("y1dc_delta_q", "y2dc_delta_q", "y2ac_delta_q", "uvdc_delta_q", "uvac_delta_q"):
            setattr(hdr_k, f, 0)
        mbs_k, coef_k = IR.to_ir({"modes": modes, "levels": levels})
        hdr = ctx.parse_into_slot(parser, write_key_frame(hdr_k, mbs_k, coef_k), 0)
        ctx.upload(0)
        r = parser.refs
        assert r.new_idx != 4
        ctx.decode([(0, r.new_idx, None)], P.STAGE_ALL)
        parser.swap(hdr)
        last = parser.refs.lst_idx
        ctx.sync()
        key = coded(ctx, last)
        rec = got["rec"][0].cpu().numpy()
        assert np.array_equal(TR.pack(key, w, h), rec), np.flatnonzero(TR.pack(key, w, h) != rec)[:8].tolist()
        assert not np.array_equal(rec, TR.pack(first, w, h))

        # the second picture: the first one moved, with a little noise, in a frame buffer the decoder does not use
        def moved(p, dy, dx):
            return TR.edge(p, dy, dx, p.shape[0], p.shape[1]).astype(np.int64)
        second = TR.noisy([((moved(p, 2 >> (i > 0), -1) + moved(p, 2 >> (i > 0), -2) + 1) >> 1).astype(np.uint8) for i, p in enumerate(first)], 5, 2)
        upload(ctx, 5, second, np.random.default_rng(1))
        jobs = [(5, last)]
        whole, _ = ctx.frames_motion(jobs, 4, planes=())
        mv, _ = ctx.frames_subpel(jobs, start=whole, planes=())
        qo = ctx.frames_quant(jobs, mv, q, filter="sixtap", stage="levels", want=("coef", "rec"))
        data, info = ctx.frames_pack(mv, qo["coef"], qindex=q, filter_level=0, cap=4096)
        frames = P.pack_frames(data, info)
        assert int(info[0, 0]) == 0 and len(frames[0]) == int(info[0, 1])
        hdr2 = ctx.parse_into_slot(parser, frames[0], 0)
        ctx.upload(0)
        r = parser.refs
        assert r.lst_idx == last and r.new_idx != 5
        ctx.decode([(0, r.new_idx, (r.lst_idx, r.gld_idx, r.alt_idx))], P.STAGE_ALL)
        ctx.sync()
        decoded = TR.pack(coded(ctx, r.new_idx), w, h)
        rec2 = qo["rec"][0].cpu().numpy()
        assert np.array_equal(decoded, rec2), np.flatnonzero(decoded != rec2)[:8].tolist()
        assert hdr2.base_qindex == q and hdr2.frame_type == 1
    finally:
        parser.close()
        ctx.close()


def test_the_wrapper(pkg, contexts):
    """shapes and types, out_* filled and returned, what the wrapper and the call refuse"""
    ctx = contexts((48, 32))
    fbs = [0, 1]
    got = ctx.frames_intra(fbs)
    assert set(got) == {"coef", "eob", "modes"} and got["coef"].dtype == torch.int16 and tuple(got["coef"].shape) == (2, 2, 3, 25, 16)
    assert got["eob"].dtype == torch.uint8 and tuple(got["eob"].shape) == (2, 2, 3, 32) and not got["eob"][..., 25:].any()
    assert got["modes"].dtype == torch.uint8 and tuple(got["modes"].shape) == (2, 2, 3, 32) and not got["modes"][..., 20:].any()
    assert int(got["modes"][..., 0].max()) <= 4 and int(got["modes"][..., 1].max()) <= 3 and int(got["modes"][..., 4:20].max()) <= 3
    outs = dict(out_coef=torch.zeros((2, 2, 3, 25, 16), dtype=torch.int16, device="cuda:0"), out_eob=torch.zeros((2, 2, 3, 32), dtype=torch.uint8, device="cuda:0"),
                out_stats=torch.zeros((2, 2, 2, 3), dtype=torch.int32, device="cuda:0"), out_rec=torch.zeros((2, 2304), dtype=torch.uint8, device="cuda:0"),
                out_modes=torch.zeros((2, 2, 3, 32), dtype=torch.uint8, device="cuda:0"))
    full = ctx.frames_intra(fbs, planes=("eobs", "recsse"), want=(), **outs)
    assert all(full[k] is outs["out_" + k] for k in OUTPUTS) and all(torch.equal(full[k], got[k]) for k in got)
    assert torch.equal(full["stats"][:, 0], got["eob"].to(torch.int32).sum(dim=3))
    for bad in (lambda: ctx.frames_intra(fbs, out_coef=outs["out_coef"].to(torch.int32)), lambda: ctx.frames_intra(fbs, out_modes=outs["out_modes"][:1]),
                lambda: ctx.frames_intra(fbs, out_stats=outs["out_stats"]), lambda: ctx.frames_intra(fbs, planes=("rd16",), out_stats=outs["out_stats"]),
                lambda: ctx.frames_intra(fbs, out_rec=outs["out_rec"][:, :-1]), lambda: ctx.frames_intra([]), lambda: ctx.frames_intra(fbs, bmode_last=10),
                lambda: ctx.frames_intra(fbs, rdmult=1001), lambda: ctx.frames_intra(fbs, rddiv=0), lambda: ctx.frames_intra(fbs, planes=("erry",)),
                lambda: ctx.frames_intra(fbs, mbmode_cost=[0, 0, 0, 0, 65536]), lambda: ctx.frames_intra(fbs, qindex=[40]),
                lambda: ctx.frames_intra(fbs, qindex=[40, 41]), lambda: ctx.frames_intra(fbs, qindex=[40, 41], rdmult=36)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(RuntimeError):
        ctx.frames_intra([4])


def test_refusals(pkg, costs):
    """every refusal of include/vp8hip.h returns -2 and writes nothing"""
    P = pkg
    ctx = P.Vp8Hip(0)
    try:
        ctx.configure(48, 32, 2, 1)
        rng = np.random.default_rng(45)
        for k in range(2):
            ctx.upload_frame(k, rng.integers(0, 256, ctx.g.frame_size, dtype=np.uint8))
        csize, esize, ssize, rsize, msize = P.intra_sizes(48, 32, ("rd16", "eobs"))
        big = torch.full((1 << 20,), 0x5C, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        d0 = big.data_ptr()
        assert d0 % 16 == 0
        dc, de, ds, dr, dm = d0, d0 + (1 << 17), d0 + (2 << 17), d0 + (3 << 17), d0 + (4 << 17)

        def call(fbs=(0, 1), pl=9, coef=dc, cs=csize, eob=de, es=esize, stats=ds, ss=ssize, rec=dr, rs=rsize, modes=dm, ms=msize, **kw):
            return raw_call(ctx, P, costs, list(fbs), planes=pl, coef=coef, coef_stride=cs, eob=eob, eob_stride=es, stats=stats, stats_stride=ss, rec=rec,
                            rec_stride=rs, modes=modes, modes_stride=ms, **kw)
        assert call(n=0) == -2 and call(n=-1) == -2
        for bad in (-1, 2, 1 << 20, -(1 << 31)):
            assert call(fbs=[bad, 0]) == -2 and call(fbs=[0, bad]) == -2, bad
        for q in (-1, 128, 1 << 20):
            assert call(q=q) == -2, q
        assert call(jq=[40, 128]) == -2 and call(jq=[255, 0]) == -2
        for k in range(5):
            for v in (-16, 16, 1 << 20):
                d = [0] * 5
                d[k] = v
                assert call(deltas=d) == -2, (k, v)
        for v in (-1, 2, 1 << 20):
            assert call(quantizer=v) == -2 and call(stage=v) == -2, v
        for k in range(3):
            for v in ((1 << 20) + 1, -(1 << 20) - 1, (1 << 31) - 1):
                z = [0] * 3
                z[k] = v
                assert call(zbin=z) == -2, (k, v)
        assert call(rdmult=-1) == -2 and call(rdmult=1001) == -2 and call(rddiv=0) == -2 and call(rddiv=101) == -2
        assert call(last=-1) == -2 and call(last=10) == -2 and call(flags=2) == -2 and call(flags=0x80000001) == -2
        for k in range(5):
            for v in (-1, 65536):
                m = [int(x) for x in costs[0]]
                m[k] = v
                assert call(mb=m) == -2, (k, v)
        for at in (0, 555, 999):
            for v in (-1, 65536):
                b = np.array(costs[1]).ravel().copy()
                b[at] = v
                assert call(bc=b) == -2, (at, v)
        assert call(pl=32) == -2 and call(pl=0x80000001) == -2 and call(pl=0) == -2                        # unknown bits; stats with planes == 0
        assert call(pl=32, stats=None) == -2
        assert call(coef=None, eob=None, stats=None, rec=None, modes=None) == -2                          # all five outputs NULL
        assert call(cs=csize - 16) == -2 and call(es=esize - 4) == -2 and call(ss=ssize - 4) == -2 and call(rs=rsize - 1) == -2 and call(ms=msize - 4) == -2
        assert call(coef=dc + 8) == -2 and call(cs=csize + 8) == -2 and call(coef=dc + 2) == -2            # coef: multiples of 16
        assert call(eob=de + 2) == -2 and call(es=esize + 2) == -2 and call(stats=ds + 2) == -2 and call(ss=ssize + 2) == -2      # eob, stats: of 4
        assert call(modes=dm + 2) == -2 and call(ms=msize + 2) == -2                                       # modes: of 4
        assert call(eob=dc + 16) == -2 and call(stats=dc + 2 * csize - 4) == -2 and call(rec=de + 5) == -2 and call(rec=ds + 3) == -2     # outputs overlap
        assert call(modes=dc) == -2 and call(modes=de + 4) == -2 and call(modes=ds) == -2 and call(modes=dr + 2 * rsize - 4) == -2
        one = lambda k: [0] * k
        none = dict(coef=None, eob=None, stats=None, rec=None, modes=None)
        assert_destinations_refused(ctx, lambda k, p, s: call(one(k), **{**none, "coef": p, "cs": s}), dc, csize, 16)
        assert_destinations_refused(ctx, lambda k, p, s: call(one(k), coef=p, cs=s), dc, csize, 16, null=False)
        assert_destinations_refused(ctx, lambda k, p, s: call(one(k), **{**none, "eob": p, "es": s}), de, esize, 4)
        assert_destinations_refused(ctx, lambda k, p, s: call(one(k), **{**none, "stats": p, "ss": s}), ds, ssize, 4)
        assert_destinations_refused(ctx, lambda k, p, s: call(one(k), **{**none, "rec": p, "rs": s}), dr, rsize, 1)
        assert_destinations_refused(ctx, lambda k, p, s: call(one(k), **{**none, "modes": p, "ms": s}), dm, msize, 4)
        ctx.sync()
        torch.cuda.synchronize()
        assert (big.cpu().numpy() == 0x5C).all()                             # nothing was enqueued
        # the same calls into memory the test owns are accepted
        assert call() == 0 and call(coef=None) == 0 and call(eob=None, stats=None) == 0 and call(rec=None, pl=31, ss=5 * 24) == 0 and call(modes=None) == 0
        assert call(stats=None, pl=0) == 0 and call(quantizer=1, stage=0, zbin=(1 << 20, -(1 << 20), 7), deltas=(-15, 15, -15, 15, -15), q=127) == 0
        assert call(jq=[0, 127]) == 0 and call(q=999, jq=[0, 127]) == 0 and call(fbs=[1, 1]) == 0 and call(rdmult=0, rddiv=100, last=9, flags=1) == 0
        assert call(rdmult=1000, rddiv=100, mb=[65535] * 5, bc=np.full(1000, 65535)) == 0                 # the ends of the ranges: inside 31 bits
        ctx.sync()
    finally:
        ctx.close()


def test_no_new_device_memory_and_inputs_untouched(pkg):
    """the call adds no device memory and writes no frame buffer"""
    P = pkg
    ctx = P.Vp8Hip(0)
    try:
        w, h = 130, 98
        ctx.configure(w, h, 2, 1)
        rng = np.random.default_rng(98)
        bufs = [rng.integers(0, 256, ctx.g.frame_size, dtype=np.uint8) for _ in range(2)]
        for k, b in enumerate(bufs):
            ctx.upload_frame(k, b)
        ctx.sync()
        rows, cols = ctx.g.aligned_h // 16, ctx.g.aligned_w // 16
        outs = dict(out_coef=torch.empty((2, rows, cols, 25, 16), dtype=torch.int16, device="cuda:0"), out_eob=torch.empty((2, rows, cols, 32), dtype=torch.uint8, device="cuda:0"),
                    out_stats=torch.empty((2, 5, rows, cols), dtype=torch.int32, device="cuda:0"),
                    out_rec=torch.empty((2, P.intra_sizes(w, h)[3]), dtype=torch.uint8, device="cuda:0"),
                    out_modes=torch.empty((2, rows, cols, 32), dtype=torch.uint8, device="cuda:0"))
        torch.cuda.synchronize()
        before, reserved = ctx.memory_usage(), torch.cuda.memory_allocated()
        for quantizer in ("regular", "fast"):
            ctx.frames_intra([0, 1], [40, 90], quantizer=quantizer, rdmult=300, rddiv=1, planes=ALL_PLANES, **outs)
            ctx.sync()
            assert ctx.memory_usage() == before and ctx.rgb_scratch_bytes() == 0 and torch.cuda.memory_allocated() == reserved
        for k, b in enumerate(bufs):
            assert np.array_equal(ctx.download_full(k), b)
    finally:
        ctx.close()
