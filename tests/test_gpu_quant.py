"""GPU (-m gpu): transform and quantisation of the motion-compensated residual of picture pairs in device memory
(vp8hip_frames_quant_async; Vp8Hip.frames_quant; csrc/hip/vp8_quant.hip), bit for bit against the numpy restatement
(tests/quant_reference.py, itself pinned to the reference's own functions by tests/test_quant_cpu.py) applied to the coded planes
vp8hip_frame_download gives: level records, dequantised levels, eobs, the five planes and the reconstruction.  The closure test holds
the reconstruction to the product's own decoder through tests/vp8_writer.py.  torch is imported here, before the package loads
libvpx's library: one HIP runtime per process."""
import ctypes
import hashlib
import json
import os
import sys

import torch  # noqa: F401  (first: the library then shares torch's HIP runtime)
import numpy as np
import pytest

from handover_testlib import assert_destinations_refused, assert_guards_intact, guarded, large_launch, picture_into
import quant_reference as QR
import scale_reference as SC
import tfilter_reference as TR
from vp8_testlib import synth_ir
from vp8_writer import write_inter_frame, write_key_frame

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from make_quant_fixtures import case_inputs  # noqa: E402

pytestmark = pytest.mark.gpu

with open(os.path.join(HERE, "golden", "quant_ref.json")) as _f:
    CASES = json.load(_f)["cases"]
OUTPUTS = ("coef", "eob", "stats", "rec")
ALL_PLANES = tuple(QR.STATS)


def case_id(c):
    return (f"{c['display'][0]}x{c['display'][1]}_{c['content']}_{c['vectors']}_q{c['qindex']}_{c['quantizer']}_{c['filter']}_" +
            "d" + ".".join(str(d) for d in c["deltas"]) + "_z" + ".".join(str(z) for z in c["zbin"]))


def coded(ctx, fb):
    """the three coded planes of a frame buffer as downloaded"""
    return [np.ascontiguousarray(p) for p in SC.planes(ctx.download_full(fb), ctx.g)]


def upload(ctx, fb, planes, rng):
    """a picture's three coded planes inside a frame buffer image of other bytes: the raster borders hold garbage"""
    ctx.upload_frame(fb, picture_into(rng.integers(0, 256, ctx.g.frame_size, dtype=np.uint8), ctx.g, planes))


def mv_on_device(mvs):
    return None if mvs is None else torch.from_numpy(np.stack(mvs).astype(np.int16)).to("cuda:0")


def expected(o, display, stage="levels", planes=ALL_PLANES):
    """the restatement's result in the call's layouts"""
    out = {"coef": o[stage], "eob": o["eob"], "rec": TR.pack(o["rec"], *display)}
    if planes:
        out["stats"] = QR.stats_tensor(o, planes)
    return out


def host(got):
    """the tensors of frames_quant as arrays (stats as the uint32 they hold)"""
    return {k: t.cpu().numpy().view(np.uint32) if k == "stats" else t.cpu().numpy() for k, t in got.items()}


def compare(got, want, i, what):
    """job i of the tensors of frames_quant (or of host() of them) against expected()"""
    for k, t in got.items():
        a = t[i] if isinstance(t, np.ndarray) else host({k: t[i:i + 1]})[k][0]
        bad = np.flatnonzero(a.ravel() != want[k].ravel())
        assert not bad.size, (what, i, k, bad[:8].tolist(), a.ravel()[bad[:8]].tolist(), want[k].ravel()[bad[:8]].tolist())


def raw_call(ctx, P, jobs, q=40, deltas=(0, 0, 0, 0, 0), quantizer=0, filt=0, stage=1, zbin=(0, 0, 0), planes=0, jq=None, mv=None, mv_stride=0, coef=None,
             coef_stride=0, eob=None, eob_stride=0, stats=None, stats_stride=0, rec=None, rec_stride=0, n=None):
    """vp8hip_frames_quant_async itself, on pointers: -> its status"""
    arr = (P.HistJob * max(len(jobs), 1))(*jobs)
    vp = ctypes.c_void_p
    keep = None if jq is None else (ctypes.c_uint8 * len(jq))(*jq)
    p = P.QuantParams(q, (ctypes.c_int * 5)(*deltas), quantizer, filt, stage, zbin[0], zbin[1], zbin[2], planes, keep)
    return ctx.L.vp8hip_frames_quant_async(ctx.h, arr, len(jobs) if n is None else n, ctypes.byref(p), vp(mv) if mv else None, mv_stride,
                                           vp(coef) if coef else None, coef_stride, vp(eob) if eob else None, eob_stride,
                                           vp(stats) if stats else None, stats_stride, vp(rec) if rec else None, rec_stride)


@pytest.fixture(scope="module")
def contexts(pkg):
    """one context of eight frame buffers per display size, shared by the tests of this module"""
    made = {}

    def get(size):
        if size not in made:
            ctx = pkg.Vp8Hip(0)
            ctx.configure(size[0], size[1], 8, 1)
            made[size] = ctx
        return made[size]
    yield get
    for ctx in made.values():
        ctx.close()


@pytest.fixture(scope="module")
def restated():
    """the restatement of a fixture case, computed once"""
    memo = {}

    def get(case):
        k = case_id(case)
        if k not in memo:
            src, ref, mv = case_inputs(case)
            memo[k] = (src, ref, mv, QR.quant_planes(src, ref, mv, case["qindex"], case["deltas"], case["quantizer"], case["filter"], case["zbin"]))
        return memo[k]
    return get


@pytest.mark.parametrize("case", [c for c in CASES if c["group"] is None], ids=case_id)
def test_fixture_cases_from_raster(pkg, contexts, restated, case):
    """every case of the fixture from uploaded frame buffers with garbage in their borders: all four outputs together, levels and
    dequantised levels"""
    display = tuple(case["display"])
    ctx = contexts(display)
    src, ref, mv, o = restated(case)
    rng = np.random.default_rng(case["seed"])
    upload(ctx, 0, src, rng)
    upload(ctx, 1, ref, rng)
    assert all(np.array_equal(a, b) for a, b in zip(coded(ctx, 0), src))
    dmv = None if mv is None else mv_on_device([mv])
    for stage in QR.STAGES:
        got = ctx.frames_quant([(0, 1)], dmv, case["qindex"], case["deltas"], case["quantizer"], case["filter"], stage, case["zbin"], ALL_PLANES,
                               want=OUTPUTS)
        assert set(got) == set(OUTPUTS)
        compare(got, expected(o, display, stage), 0, (case_id(case), stage))


def test_job_qindex_and_each_output_alone(pkg, contexts, restated):
    """a qindex a job (the fixture's group of four pairs under one set of deltas); each output alone, in pairs and all together give the same
    bytes; a call without rec and RECSSE; twice for determinism"""
    group = [c for c in CASES if c["group"] == "jobq"]
    ctx = contexts((32, 32))
    rng = np.random.default_rng(3)
    jobs, mvs, wants, qs = [], [], [], []
    for i, c in enumerate(group):
        src, ref, mv, o = restated(c)
        upload(ctx, 2 * i, src, rng)
        upload(ctx, 2 * i + 1, ref, rng)
        jobs.append((2 * i, 2 * i + 1))
        mvs.append(mv)
        wants.append(expected(o, (32, 32)))
        qs.append(c["qindex"])
    assert len(set(qs)) == 4
    dmv = mv_on_device(mvs)
    kw = dict(deltas=group[0]["deltas"], quantizer=group[0]["quantizer"], filter=group[0]["filter"], zbin=group[0]["zbin"])
    full = ctx.frames_quant(jobs, dmv, qs, planes=ALL_PLANES, want=OUTPUTS, **kw)
    again = ctx.frames_quant(jobs, dmv, qs, planes=ALL_PLANES, want=OUTPUTS, **kw)
    for i in range(len(jobs)):
        compare(host(full), wants[i], i, "job_qindex")
    assert all(torch.equal(full[k], again[k]) for k in OUTPUTS)
    for want in (("coef",), ("eob",), ("rec",), ("coef", "eob"), ("eob", "rec")):
        got = ctx.frames_quant(jobs, dmv, qs, want=want, **kw)
        assert set(got) == set(want) and all(torch.equal(got[k], full[k]) for k in want), want
    for planes in (("erry",), ("recsse",), ("eobs", "erry2"), ("erruv", "erry", "eobs")):          # stats alone; without and with the inverse side
        got = ctx.frames_quant(jobs, dmv, qs, planes=planes, want=(), **kw)
        assert set(got) == {"stats"} and tuple(got["stats"].shape) == (4, len(planes), 2, 2)
        bits = [list(QR.STATS).index(p) for p in sorted(planes, key=list(QR.STATS).index)]
        assert torch.equal(got["stats"], full["stats"][:, bits]), planes
    one = ctx.frames_quant(jobs[:1], dmv[:1], qs[0], want=("coef",), stage="dequant", **kw)        # a scalar qindex; the other stage
    assert np.array_equal(one["coef"][0].cpu().numpy(), QR.quant_planes(*case_inputs(group[0]), qs[0], group[0]["deltas"])["dequant"])


def test_strides_and_alignment(pkg, contexts, restated):
    """every output with bytes between the jobs and at the least alignment it allows: the values, and the bytes around them"""
    case = next(c for c in CASES if tuple(c["display"]) == (67, 45) and c["content"] == "decoded")
    ctx = contexts((67, 45))
    src, ref, mv, o = restated(case)
    rng = np.random.default_rng(11)
    upload(ctx, 0, src, rng)
    upload(ctx, 1, ref, rng)
    jobs = [(0, 1), (0, 0), (0, 1)]
    self_o = QR.quant_planes(src, src, mv, case["qindex"], case["deltas"], case["quantizer"], case["filter"], case["zbin"])
    wants = [expected(o, (67, 45)), expected(self_o, (67, 45)), expected(o, (67, 45))]
    dmv = mv_on_device([mv] * 3)
    csize, esize, ssize, rsize = pkg.quant_sizes(67, 45, ALL_PLANES)
    assert (csize, esize, ssize) == (800 * 15, 32 * 15, 4 * 5 * 15)
    for (coff, cpad), (eoff, epad), (soff, spad), (roff, rpad) in (((16, 0), (4, 0), (4, 0), (1, 0)), ((48, 16), (12, 4), (8, 12), (3, 5)),
                                                                    ((0, 160), (0, 32), (0, 4), (7, 1))):
        cbig, cflat = guarded(3, csize, cpad, coff)
        ebig, eflat = guarded(3, esize, epad, eoff)
        sbig, sflat = guarded(3, ssize, spad, soff)
        rbig, rflat = guarded(3, rsize, rpad, roff)
        torch.cuda.synchronize()
        assert raw_call(ctx, pkg, jobs, case["qindex"], case["deltas"], QR.QUANTIZERS.index(case["quantizer"]), TR.FILTERS.index(case["filter"]), 1,
                        case["zbin"], 31, None, dmv.data_ptr(), dmv.stride(0) * 2, cflat.data_ptr(), csize + cpad, eflat.data_ptr(), esize + epad,
                        sflat.data_ptr(), ssize + spad, rflat.data_ptr(), rsize + rpad) == 0
        ctx.sync()
        for i in range(3):
            got = {"coef": cflat.cpu().numpy()[i].view(np.int16), "eob": eflat.cpu().numpy()[i], "stats": sflat.cpu().numpy()[i].view(np.uint32),
                   "rec": rflat.cpu().numpy()[i]}
            for k, a in got.items():
                assert np.array_equal(a.ravel(), wants[i][k].ravel()), (k, i, coff, cpad)
        assert_guards_intact(cbig, 3, csize, cpad, coff, what="coef")
        assert_guards_intact(ebig, 3, esize, epad, eoff, what="eob")
        assert_guards_intact(sbig, 3, ssize, spad, soff, what="stats")
        assert_guards_intact(rbig, 3, rsize, rpad, roff, what="rec")


def test_vectors_from_frames_subpel_and_int16_ends(pkg, contexts):
    """frames_motion -> frames_subpel -> frames_quant with the tensor passed on untouched; then the ends of int16"""
    ctx = contexts((176, 144))
    src, ref = QR.pictures("decoded", 176, 144, 77, k=4)
    rng = np.random.default_rng(5)
    upload(ctx, 0, src, rng)
    upload(ctx, 1, ref, rng)
    jobs = [(0, 1), (1, 0)]
    whole, _ = ctx.frames_motion(jobs, 4, planes=())
    mv, _ = ctx.frames_subpel(jobs, start=whole, planes=())
    got = ctx.frames_quant(jobs, mv, 40, planes=ALL_PLANES, want=OUTPUTS)
    mvs = mv.cpu().numpy().astype(np.int64)
    assert (mvs & 7).any() and (mvs < 0).any()
    for i, (a, b) in enumerate(((src, ref), (ref, src))):
        compare(got, expected(QR.quant_planes(a, b, mvs[i], 40), (176, 144)), i, "subpel")
    ends = np.zeros((2, 2, 9, 11), np.int64)
    ends[0, 0], ends[0, 1], ends[1, 0], ends[1, 1] = 32767, -32768, -32768, 32767
    ends[1, 0, :, ::2], ends[1, 1, ::2] = 32766, -32767
    for filt in TR.FILTERS:
        got = ctx.frames_quant(jobs, mv_on_device(list(ends)), 40, filter=filt, planes=ALL_PLANES, want=OUTPUTS)
        for i, (a, b) in enumerate(((src, ref), (ref, src))):
            compare(got, expected(QR.quant_planes(a, b, ends[i], 40, filt=filt), (176, 144)), i, ("ends", filt))


def test_many_jobs_cross_the_launch_limits(pkg, contexts):
    """more jobs than a launch takes (160), and more different qindex values than it has tables (8), in any order with repeats"""
    ctx = contexts((32, 32))
    rng = np.random.default_rng(8)
    pics = [TR.picture("smooth", 32, 32, 1), TR.picture("noise", 32, 32, 2), TR.picture("smooth", 32, 32, 3), TR.picture("flat97", 32, 32, 0)]
    for fb, p in enumerate(pics):
        upload(ctx, fb, p, rng)
    pairs = [(0, 1), (0, 2), (2, 0), (3, 0), (1, 1)]
    memo = {}

    def want(pair, q, mv):
        k = (pair, q)
        if k not in memo:
            memo[k] = expected(QR.quant_planes(pics[pair[0]], pics[pair[1]], mv, q), (32, 32))
        return memo[k]
    mv = TR.fixture_mv("phases", 2, 2, 9)
    for n, qs in ((400, [40, 3, 127]), (60, list(range(0, 120, 6)))):
        jobs = [pairs[int(k)] for k in rng.integers(0, len(pairs), n)]
        jq = [qs[int(k)] for k in rng.integers(0, len(qs), n)]
        got = host(ctx.frames_quant(jobs, mv_on_device([mv] * n), jq, planes=ALL_PLANES, want=OUTPUTS))
        for i in range(n):
            compare(got, want(jobs[i], jq[i], mv), i, (n, jobs[i], jq[i]))


@pytest.mark.parametrize("name", ["kf_odd_67x45", "kf_q0_176x144"])
def test_jobs_from_tiles(pkg, name, monkeypatch):
    """frames a large launch left as tiles: source and reference as tiles, tiles mixed with an uploaded raster frame in both roles, a
    frame against itself, a frame buffer never written; no raster pool is made for them and the context's memory does not change.
    Expected values from pictures downloaded AFTER the calls: a download gives a tiled frame its raster form"""
    P = pkg
    n = 3
    ctx = P.Vp8Hip(0)
    try:
        nsrc = large_launch(P, ctx, name, n, monkeypatch)
        ctx.sync()
        assert ctx.memory_usage()["raster_pool"] == 0 and ctx.memory_usage()["tile_pool"] > 0
        before = ctx.memory_usage()
        rows, cols = ctx.g.aligned_h // 16, ctx.g.aligned_w // 16
        jobs = [(0, 1), (1, 0), (2, 2), (n + 1, 0), (0, n + 1)]
        mvs = [TR.fixture_mv("phases", rows, cols, 51, k) for k in range(len(jobs))]
        dmv = mv_on_device(mvs)
        first = [ctx.frames_quant(jobs, dmv, 40, filter=f, planes=ALL_PLANES, want=OUTPUTS) for f in TR.FILTERS]
        ctx.sync()
        assert ctx.memory_usage() == before                                  # no raster pool, nothing else
        ctx.upload_frame(n, np.random.default_rng(67).integers(0, 256, ctx.g.frame_size, dtype=np.uint8))     # raster only
        before = ctx.memory_usage()
        mixed_jobs = [(0, n), (n, 1), (n, n)]
        mixed = ctx.frames_quant(mixed_jobs, dmv[:3], 3, deltas=(0, 1, 0, 0, 0), quantizer="fast", planes=ALL_PLANES, want=OUTPUTS)
        ctx.sync()
        assert ctx.memory_usage() == before
        never = [np.zeros((ctx.g.aligned_h >> s, ctx.g.aligned_w >> s), np.uint8) for s in (0, 1, 1)]
        pics = {k: coded(ctx, k) for k in range(n + 1)}
        pics[n + 1] = never
        display = (ctx.width, ctx.height)
        assert nsrc < 2 or not np.array_equal(pics[0][0], pics[1][0])
        for got, f in zip(first, TR.FILTERS):
            for i, (a, b) in enumerate(jobs):
                compare(got, expected(QR.quant_planes(pics[a], pics[b], mvs[i], 40, filt=f), display), i, (name, f, "tiles"))
        for i, (a, b) in enumerate(mixed_jobs):
            compare(mixed, expected(QR.quant_planes(pics[a], pics[b], mvs[i], 3, (0, 1, 0, 0, 0), "fast"), display), i, (name, "mixed"))
        after = ctx.frames_quant(jobs, dmv, 40, planes=ALL_PLANES, want=OUTPUTS)                 # ... every frame in raster form
        assert all(torch.equal(after[k], first[0][k]) for k in OUTPUTS)
    finally:
        ctx.close()


def test_closure_with_the_writer_and_the_decoder(pkg):
    """the call plus an entropy coder is a VP8 encoder: a key frame and a second picture at 48x32; frames_motion (d = 4),
    frames_subpel, frames_quant at qindex 40 (six-tap, levels); an IR of NEWMV macroblocks from the vectors and the transposed
    levels, written by vp8_writer.write_inter_frame with loop filter level 0 and decoded by the product: the decoded frame equals
    rec byte for byte"""
    P = pkg
    w, h, q = 48, 32, 40
    rows, cols = 2, 3
    hdr_k, mbs_k, coef_k, _ = synth_ir(w, h, 21, inter=False, dense=0.3, segmented=False)
    hdr_k.filter_level = 0
    ctx = P.Vp8Hip(0)
    parser = P.Parser()
    try:
        ctx.configure(w, h, 6, 1)
        hdr = ctx.parse_into_slot(parser, write_key_frame(hdr_k, mbs_k, coef_k), 0)
        ctx.upload(0)
        r = parser.refs
        ctx.decode([(0, r.new_idx, None)], P.STAGE_ALL)
        parser.swap(hdr)
        last = parser.refs.lst_idx
        ctx.sync()
        key = coded(ctx, last)
        # the second picture: the key frame moved by (2, -1.5) pixels (the mean of two whole-pixel moves) with a little noise and a
        # brightness ramp (so that Y2 blocks are coded too), in a frame buffer the decoder does not use
        def moved(p, dy, dx):
            return TR.edge(p, dy, dx, p.shape[0], p.shape[1]).astype(np.int64)
        second = TR.noisy([((moved(p, 2 >> (i > 0), -1) + moved(p, 2 >> (i > 0), -2) + 1) >> 1).astype(np.uint8) for i, p in enumerate(key)], 5, 2)
        second[0] = np.clip(second[0].astype(np.int64) + 4 + np.arange(w) // 8, 0, 255).astype(np.uint8)
        upload(ctx, 5, second, np.random.default_rng(1))
        jobs = [(5, last)]
        whole, _ = ctx.frames_motion(jobs, 4, planes=())
        mv, _ = ctx.frames_subpel(jobs, start=whole, planes=())
        got = ctx.frames_quant(jobs, mv, q, filter="sixtap", stage="levels", want=("coef", "eob", "rec"))
        levels = got["coef"][0].cpu().numpy().reshape(rows * cols, 25, 4, 4)
        vec = mv[0].cpu().numpy().astype(np.int64)
        assert levels[:, :24].any() and levels[:, 24].any() and (vec & 7).any()                 # something is coded; some vector is fractional
        # the IR: every macroblock inter, NEWMV from the last frame, not skipped; a block is the transpose of the call's
        hdr_i, mbs, coef, mvs = synth_ir(w, h, 22, inter=True, segmented=False)
        hdr_i.base_qindex, hdr_i.filter_level, hdr_i.refresh_last, hdr_i.show_frame, hdr_i.version, hdr_i.mode_ref_lf_delta_enabled = q, 0, 1, 1, 0, 0
        for f in ("y1dc_delta_q", "y2dc_delta_q", "y2ac_delta_q", "uvdc_delta_q", "uvac_delta_q"):
            setattr(hdr_i, f, 0)
        mbs[:] = 0
        mbs[:, 0], mbs[:, 2] = 8, 1
        coef[:] = levels.transpose(0, 1, 3, 2).reshape(rows * cols, 400)
        coef[:, 0:256:16] = 0                                               # position 0 of the luma blocks is not coded: the Y2 block carries it
        mvs[:, :, 0], mvs[:, :, 1] = vec[1].reshape(-1, 1), vec[0].reshape(-1, 1)                # (row, column)
        data, mbs2, mvs2 = write_inter_frame(hdr_i, mbs, coef, mvs)
        assert np.array_equal(mvs2, mvs) and not (mbs2[:, 3] & 2).any() and (mbs2[:, 0] == 8).all()   # the writer carried every vector as it is, unclamped
        hdr2 = ctx.parse_into_slot(parser, data, 0)
        ctx.upload(0)
        r = parser.refs
        assert r.lst_idx == last and r.new_idx != 5
        ctx.decode([(0, r.new_idx, (r.lst_idx, r.gld_idx, r.alt_idx))], P.STAGE_ALL)
        ctx.sync()
        decoded = TR.pack(coded(ctx, r.new_idx), w, h)
        rec = got["rec"][0].cpu().numpy()
        assert np.array_equal(decoded, rec), np.flatnonzero(decoded != rec)[:8].tolist()
        assert not np.array_equal(rec, TR.pack(second, w, h)) and hdr2.base_qindex == q           # (quantised: not the source itself)
    finally:
        parser.close()
        ctx.close()


def test_the_wrapper(pkg, contexts):
    """shapes and types, out_* filled and returned, what the wrapper and the call refuse"""
    P = pkg
    ctx = contexts((48, 32))
    jobs = [(0, 1), (1, 0)]
    got = ctx.frames_quant(jobs)
    assert set(got) == {"coef", "eob"} and got["coef"].dtype == torch.int16 and tuple(got["coef"].shape) == (2, 2, 3, 25, 16)
    assert got["eob"].dtype == torch.uint8 and tuple(got["eob"].shape) == (2, 2, 3, 32) and not got["eob"][..., 25:].any()
    outs = dict(out_coef=torch.zeros((2, 2, 3, 25, 16), dtype=torch.int16, device="cuda:0"), out_eob=torch.zeros((2, 2, 3, 32), dtype=torch.uint8, device="cuda:0"),
                out_stats=torch.zeros((2, 2, 2, 3), dtype=torch.int32, device="cuda:0"), out_rec=torch.zeros((2, 2304), dtype=torch.uint8, device="cuda:0"))
    full = ctx.frames_quant(jobs, planes=("eobs", "recsse"), want=(), **outs)
    assert all(full[k] is outs["out_" + k] for k in OUTPUTS) and torch.equal(full["coef"], got["coef"]) and torch.equal(full["eob"], got["eob"])
    assert torch.equal(full["stats"][:, 0], got["eob"].to(torch.int32).sum(dim=3))
    y, u, v = P.split_i420(full["rec"], 48, 32)
    assert tuple(y.shape) == (2, 32, 48) and tuple(u.shape) == (2, 16, 24) == tuple(v.shape)
    mv = torch.zeros((2, 2, 2, 3), dtype=torch.int16, device="cuda:0")
    assert torch.equal(ctx.frames_quant(jobs, mv)["coef"], got["coef"])
    for bad in (lambda: ctx.frames_quant(jobs, out_coef=outs["out_coef"].to(torch.int32)), lambda: ctx.frames_quant(jobs, out_coef=outs["out_coef"][:1]),
                lambda: ctx.frames_quant(jobs, out_eob=outs["out_eob"].to(torch.int16)), lambda: ctx.frames_quant(jobs, out_stats=outs["out_stats"]),
                lambda: ctx.frames_quant(jobs, planes=("erry",), out_stats=outs["out_stats"]), lambda: ctx.frames_quant(jobs, out_rec=outs["out_rec"][:, :-1]),
                lambda: ctx.frames_quant(jobs, mv=mv[:1]), lambda: ctx.frames_quant(jobs, mv=mv.to(torch.int32)), lambda: ctx.frames_quant(jobs, mv=mv.cpu())):
        with pytest.raises(ValueError):
            bad()
    for bad in (lambda: ctx.frames_quant([(0, 8)]), lambda: ctx.frames_quant([(8, 0)])):
        with pytest.raises(RuntimeError):
            bad()


def test_refusals(pkg):
    """every refusal of include/vp8hip.h returns -2 and writes nothing"""
    P = pkg
    ctx = P.Vp8Hip(0)
    try:
        ctx.configure(48, 32, 2, 1)
        rng = np.random.default_rng(45)
        for k in range(2):
            ctx.upload_frame(k, rng.integers(0, 256, ctx.g.frame_size, dtype=np.uint8))
        csize, esize, ssize, rsize = P.quant_sizes(48, 32, ("erry", "eobs"))
        msize = 24
        big = torch.full((1 << 20,), 0x5C, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        d0 = big.data_ptr()
        assert d0 % 16 == 0
        dc, de, ds, dr, dm = d0, d0 + (1 << 17), d0 + (2 << 17), d0 + (3 << 17), d0 + (4 << 17)

        def call(jobs=((0, 1), (1, 0)), q=40, deltas=(0, 0, 0, 0, 0), qz=0, f=0, st=1, zb=(0, 0, 0), pl=9, jq=None, mv=None, ms=msize, coef=dc, cs=csize, eob=de,
                 es=esize, stats=ds, ss=ssize, rec=dr, rs=rsize, n=None):
            return raw_call(ctx, P, list(jobs), q, deltas, qz, f, st, zb, pl, jq, mv, ms, coef, cs, eob, es, stats, ss, rec, rs, n)
        assert call(n=0) == -2 and call(n=-1) == -2
        for bad in (-1, 2, 1 << 20, -(1 << 31)):
            assert call(jobs=[(bad, 0)]) == -2 and call(jobs=[(0, bad)]) == -2, bad
        for q in (-1, 128, 1 << 20):
            assert call(q=q) == -2, q
        assert call(jq=[40, 128]) == -2 and call(jq=[255, 0]) == -2
        for k in range(5):
            for v in (-16, 16, 1 << 20):
                d = [0] * 5
                d[k] = v
                assert call(deltas=d) == -2, (k, v)
        for v in (-1, 2, 1 << 20):
            assert call(qz=v) == -2 and call(f=v) == -2 and call(st=v) == -2, v
        for k in range(3):
            for v in ((1 << 20) + 1, -(1 << 20) - 1, (1 << 31) - 1):
                z = [0] * 3
                z[k] = v
                assert call(zb=z) == -2, (k, v)
        assert call(pl=32) == -2 and call(pl=0x80000001) == -2 and call(pl=0) == -2                        # unknown bits; stats with planes == 0
        assert call(pl=32, stats=None) == -2                                                              # unknown bits even where stats is NULL
        assert call(coef=None, eob=None, stats=None, rec=None) == -2                                      # all four outputs NULL
        assert call(cs=csize - 16) == -2 and call(es=esize - 4) == -2 and call(ss=ssize - 4) == -2 and call(rs=rsize - 1) == -2
        assert call(mv=dm, ms=msize - 2) == -2
        assert call(coef=dc + 8) == -2 and call(cs=csize + 8) == -2 and call(coef=dc + 2) == -2            # coef: multiples of 16
        assert call(eob=de + 2) == -2 and call(es=esize + 2) == -2 and call(stats=ds + 2) == -2 and call(ss=ssize + 2) == -2      # eob, stats: of 4
        assert call(mv=dm + 1) == -2 and call(mv=dm, ms=msize + 1) == -2                                   # mv: of 2
        assert call(eob=dc + 16) == -2 and call(stats=dc + 2 * csize - 4) == -2 and call(rec=de + 5) == -2 and call(rec=ds + 3) == -2     # outputs overlap
        assert call(mv=dc) == -2 and call(mv=de + 2) == -2 and call(mv=ds) == -2 and call(mv=dr + 2 * rsize - 2) == -2                   # ... or the vectors
        one = lambda k: [(0, 1)] * k
        assert_destinations_refused(ctx, lambda k, p, s: call(one(k), coef=p, cs=s, eob=None, stats=None, rec=None), dc, csize, 16)
        assert_destinations_refused(ctx, lambda k, p, s: call(one(k), coef=p, cs=s), dc, csize, 16, null=False)
        assert_destinations_refused(ctx, lambda k, p, s: call(one(k), eob=p, es=s, coef=None, stats=None, rec=None), de, esize, 4)
        assert_destinations_refused(ctx, lambda k, p, s: call(one(k), stats=p, ss=s, coef=None, eob=None, rec=None), ds, ssize, 4)
        assert_destinations_refused(ctx, lambda k, p, s: call(one(k), rec=p, rs=s, coef=None, eob=None, stats=None), dr, rsize, 1)
        assert_destinations_refused(ctx, lambda k, p, s: call(one(k), mv=p, ms=s), dm, msize, 2, null=False)
        ctx.sync()
        torch.cuda.synchronize()
        assert (big.cpu().numpy() == 0x5C).all()                             # nothing was enqueued
        # the same calls into memory the test owns are accepted
        big[4 << 17:(4 << 17) + 2 * msize] = 0
        torch.cuda.synchronize()
        assert call() == 0 and call(mv=dm) == 0 and call(coef=None) == 0 and call(eob=None, stats=None) == 0 and call(rec=None, pl=31, ss=5 * 24) == 0
        assert call(stats=None, pl=0) == 0 and call(qz=1, f=1, st=0, zb=(1 << 20, -(1 << 20), 7), deltas=(-15, 15, -15, 15, -15), q=127) == 0
        assert call(jq=[0, 127]) == 0 and call(q=999, jq=[0, 127]) == 0 and call(jobs=[(0, 0), (1, 1)]) == 0      # (qindex is not read beside job_qindex)
        ctx.sync()
    finally:
        ctx.close()


def test_no_new_device_memory_and_inputs_untouched(pkg):
    """the call adds no device memory; no frame buffer and no input tensor is written"""
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
                    out_rec=torch.empty((2, P.quant_sizes(w, h)[3]), dtype=torch.uint8, device="cuda:0"))
        mv = torch.full((2, 2, rows, cols), 21, dtype=torch.int16, device="cuda:0")
        torch.cuda.synchronize()
        md5 = [hashlib.md5(ctx.download_full(k).tobytes()).hexdigest() for k in range(2)]
        before, reserved = ctx.memory_usage(), torch.cuda.memory_allocated()
        for quantizer in QR.QUANTIZERS:
            ctx.frames_quant([(0, 1), (1, 1)], mv, [40, 90], quantizer=quantizer, planes=ALL_PLANES, **outs)
            ctx.sync()
            assert ctx.memory_usage() == before and ctx.rgb_scratch_bytes() == 0 and torch.cuda.memory_allocated() == reserved
        for k, b in enumerate(bufs):
            got = ctx.download_full(k)
            assert np.array_equal(got, b) and hashlib.md5(got.tobytes()).hexdigest() == md5[k]
        assert (mv.cpu().numpy() == 21).all()
    finally:
        ctx.close()
