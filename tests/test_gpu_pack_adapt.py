"""GPU (-m gpu): compressed VP8 inter frames with probabilities adapted to each frame's own counts (vp8hip_frames_pack_adapt_async;
Vp8Hip.frames_pack_adapt; csrc/hip/vp8_pack_adapt.hip), against the restatement (tests/pack_adapt_reference.py, which
tests/test_pack_adapt_cpu.py holds to the reference's functions and to the real reference decoder): the frame's bytes, info, counts
and probs_out entry for entry.  The chain test puts the call behind frames_motion, frames_subpel and frames_quant and decodes a
stream of three frames with the product's own decoder.  torch is imported here, before the package loads libvpx's library: one HIP
runtime per process."""
import ctypes

import torch  # noqa: F401  (first: the library then shares torch's HIP runtime)
import numpy as np
import pytest

from handover_testlib import assert_destinations_refused, assert_guards_intact, guarded, picture_into
import pack_adapt_reference as A
import pack_reference as R
import scale_reference as SC
import tfilter_reference as TR
from vp8_testlib import synth_ir
from vp8_writer import write_key_frame

pytestmark = pytest.mark.gpu
GUARD = 64


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
    """the restatement of (content key, parameters), computed once"""
    memo = {}

    def get(key, mv, lv, probs_in=None, **kw):
        k = (key, tuple(sorted(kw.items())), None if probs_in is None else probs_in.tobytes())
        if k not in memo:
            memo[k] = A.restate(mv, lv, probs_in=probs_in, **kw)
        return memo[k]
    return get


def content(rows, cols, field, levels, seed):
    return R.make_field(field, rows, cols, seed), R.make_levels(levels, rows, cols, seed)


def other_probs(seed):
    """a baseline set that is not the default one: every probability moved, inside 1..255"""
    rng = np.random.default_rng(seed)
    p = A.default_probs().astype(np.int64)
    p[:1094] = np.clip(p[:1094] + rng.integers(-40, 41, size=1094), 1, 255)
    return p.astype(np.uint8)


def fenced(n, width, dtype, fill):
    """-> (big, view): a contiguous [n, width] tensor inside a larger one of `fill`, GUARD elements on both sides"""
    big = torch.full((n * width + 2 * GUARD,), fill, dtype=dtype, device="cuda:0")
    return big, big[GUARD:GUARD + n * width].view(n, width)


def fence_intact(big, n, width, fill):
    a = big.cpu().numpy()
    return (a[:GUARD] == fill).all() and (a[GUARD + n * width:] == fill).all()


def pack(ctx, jobs, cap=None, pad=48, qindex=40, probs_in=None, **kw):
    """frames_pack_adapt over jobs = [(mv or None, levels)] into guarded memory -> (data, info, counts, probs) as arrays; the
    guards around every job's dst and around info, counts and probs_out are checked.  probs_in: None, uint8 [1104] or [n, 1104]"""
    n = len(jobs)
    rows, cols = jobs[0][1].shape[:2]
    cap = ctx.pack_adapt_bound(kw.get("log2_parts", 0)) if cap is None else cap
    big, data = guarded(n, cap, pad, 64)
    bi, info = fenced(n, 32, torch.int32, -1515870811)
    bc, counts = fenced(n, A.COUNTS, torch.int32, -1515870811)
    bp, probs = fenced(n, A.PROBS_BYTES, torch.uint8, 0xA5)
    coef = torch.from_numpy(np.stack([j[1] for j in jobs]).astype(np.int16)).to("cuda:0")
    mvt = None
    if not all(j[0] is None for j in jobs):
        mvt = torch.from_numpy(np.stack([np.zeros((2, rows, cols), np.int16) if j[0] is None else j[0] for j in jobs]).astype(np.int16)).to("cuda:0")
    pin = None
    if probs_in is not None:
        pin = torch.from_numpy(np.ascontiguousarray(probs_in)).to("cuda:0")
    d, i, c, p = ctx.frames_pack_adapt(mvt, coef, qindex=qindex, cap=cap, probs_in=pin, out_data=data, out_info=info, out_counts=counts, out_probs=probs, **kw)
    assert d is data and i is info and c is counts and p is probs
    torch.cuda.synchronize()
    assert_guards_intact(big, n, cap, pad, 64, what="bytes outside the jobs' regions were written")
    assert fence_intact(bi, n, 32, -1515870811) and fence_intact(bc, n, A.COUNTS, -1515870811) and fence_intact(bp, n, A.PROBS_BYTES, 0xA5)
    return data.cpu().numpy(), info.cpu().numpy().astype(np.int64), counts.cpu().numpy().astype(np.int64), probs.cpu().numpy()


def same(got, i, want, what):
    """job i of pack() against a restatement: info, bytes, counts and probs_out entry for entry"""
    data, info, counts, probs = got
    assert info[i].tolist() == want["info"].tolist(), (what, i, info[i].tolist(), want["info"].tolist())
    assert np.array_equal(counts[i], want["counts"]), (what, i, np.flatnonzero(counts[i] != want["counts"])[:8].tolist())
    assert np.array_equal(probs[i], want["probs_out"]), (what, i, np.flatnonzero(probs[i] != want["probs_out"])[:8].tolist())
    if want["data"] is not None:
        frame = data[i, :info[i, 1]].tobytes()
        bad = [k for k in range(min(len(frame), len(want["data"]))) if frame[k] != want["data"][k]][:8]
        assert frame == want["data"], (what, i, len(frame), len(want["data"]), bad)


@pytest.mark.parametrize("size,display,lp,keys", [
    ((48, 32), (48, 32), 0, [("alphabet", "sparse"), ("far", "dense"), ("zero", "zero"), ("equal", "edges")]),
    ((48, 32), (48, 32), 1, [("alphabet", "dense"), ("far", "sparse")]),
    ((48, 32), (48, 32), 2, [("alphabet", "edges"), ("zero", "sparse")]),
    ((48, 32), (48, 32), 3, [("far", "edges"), ("equal", "dense")]),
    ((16, 16), (16, 16), 0, [("alphabet", "dense"), ("zero", "zero"), ("far", "edges"), ("equal", "sparse")]),
    ((80, 48), (67, 45), 1, [("alphabet", "sparse"), ("far", "dense"), ("equal", "edges")]),
    ((176, 144), (176, 144), 3, [("alphabet", "dense"), ("far", "sparse"), ("zero", "zero")]),
    ((176, 144), (176, 144), 0, [("alphabet", "sparse"), ("equal", "edges")]),
], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_sizes_partitions_and_contents(pkg, contexts, restated, size, display, lp, keys):
    """all flags, at four sizes, 1 to 8 partitions, zero, sparse and dense levels, every kind of vector field"""
    ctx = contexts(display)
    rows, cols = size[1] // 16, size[0] // 16
    jobs = [content(rows, cols, f, l, 31 + k) for k, (f, l) in enumerate(keys)]
    got = pack(ctx, jobs, log2_parts=lp)
    for i, ((f, l), (mv, lv)) in enumerate(zip(keys, jobs)):
        want = restated((size, f, l, i), mv, lv, log2_parts=lp)
        same(got, i, want, (size, f, l, lp))
        if l == "dense" and rows * cols > 1:
            assert got[1][i, 16] > 0 and got[1][i, 19] > 0                      # the tables are fitted ...
            assert got[1][i, 1] < len(want["default"])                          # ... and the frame is smaller for it
        if f == "far" and rows * cols > 50:
            assert got[1][i, 17] > 0                                            # long differences: vector probabilities are updated
    assert ctx.pack_adapt_bound(lp) == pkg.pack_adapt_bound(display[0], display[1], lp) == ctx.pack_bound(lp) + 8624


def test_one_macroblock_where_nothing_pays(contexts, restated):
    """a single small level: no update is worth its bits"""
    lv = np.zeros((1, 1, 25, 16), np.int16)
    lv[0, 0, 24, 0] = 1
    got = pack(contexts((16, 16)), [(None, lv)])
    same(got, 0, restated("nothing pays", None, lv), "16x16")
    assert got[1][0, 16] == 0 and got[1][0, 17] == 0 and got[1][0, 19] == 0 and got[1][0, 18] == 255
    assert np.array_equal(got[3][0], A.default_probs()) and got[2][0].sum() == 2 + 16 + 8       # a token and an end of block; 24 ends of block


def test_an_all_skipped_frame(contexts, restated):
    """no level at all: prob_skip_false clips to 1 and every count is zero"""
    mv, lv = content(2, 3, "zero", "zero", 3)
    got = pack(contexts((48, 32)), [(mv, lv)])
    same(got, 0, restated("all skipped", mv, lv), "all skipped")
    assert got[1][0, 18] == 1 and got[1][0, 11] == 6 and not got[2][0].any()


def test_vector_counts(contexts, restated):
    """no NEWMV at all: the vector counts are zero and nothing is updated; many NEWMV with long differences: updates"""
    ctx = contexts((176, 144))
    calm, far = content(9, 11, "zero", "sparse", 8), content(9, 11, "far", "sparse", 897)
    got = pack(ctx, [calm, far], log2_parts=1)
    same(got, 0, restated("calm", *calm, log2_parts=1), "calm")
    same(got, 1, restated("far", *far, log2_parts=1), "far")
    assert got[1][0, 15] == 0 and not got[2][0, 1152:].any() and got[1][0, 17] == 0 and got[1][1, 15] > 90
    assert got[2][1, 1152 + 1] > 50 and got[2][1, 1152 + 32 + 1] > 50 and got[1][1, 17] >= 4    # long forms counted in both components


@pytest.mark.parametrize("refresh", (0, 1))
def test_every_flag_alone_and_all_together(contexts, restated, refresh):
    ctx = contexts((176, 144))
    job = content(9, 11, "far", "sparse", 897)
    sizes = {}
    for flags in (0, A.COEF, A.MV, A.SKIP, A.REF, A.ALL):
        got = pack(ctx, [job], flags=flags, refresh_entropy_probs=refresh, log2_parts=1, ref_frame=2, cap=16384)
        want = restated("flags", *job, flags=flags, refresh_entropy_probs=refresh, log2_parts=1, ref_frame=2)
        same(got, 0, want, (flags, refresh))
        sizes[flags] = got[1][0, 1]
        assert (got[1][0, 16] > 0) == bool(flags & A.COEF) and (got[1][0, 17] > 0) == bool(flags & A.MV)
        assert got[1][0, 18] == (want["info"][18] if flags & A.SKIP else 200) != 0
    assert all(sizes[f] < sizes[0] for f in (A.COEF, A.MV, A.REF, A.ALL)) and sizes[A.ALL] == min(sizes.values())


def test_no_flags_and_defaults_is_frames_pack(contexts):
    """with no flags, the default baseline and refresh_entropy_probs 1: the bytes and info[0..15] of frames_pack for the same inputs"""
    ctx = contexts((48, 32))
    jobs = [content(2, 3, f, l, 50 + k) for k, (f, l) in enumerate((("alphabet", "sparse"), ("far", "dense"), ("zero", "zero"), ("equal", "edges")))]
    data, info, counts, probs = pack(ctx, jobs, flags=0, log2_parts=1, prob_skip_false=77, cap=8192)
    coef = torch.from_numpy(np.stack([j[1] for j in jobs])).to("cuda:0")
    mv = torch.from_numpy(np.stack([j[0] for j in jobs])).to("cuda:0")
    d0, i0 = ctx.frames_pack(mv, coef, log2_parts=1, prob_skip_false=77, cap=8192)
    d0, i0 = d0.cpu().numpy(), i0.cpu().numpy().astype(np.int64)
    for i in range(len(jobs)):
        assert info[i, :16].tolist() == i0[i].tolist() and info[i, 16:].tolist() == [0, 0, 77, 0] + [0] * 12
        assert data[i, :info[i, 1]].tobytes() == d0[i, :i0[i, 1]].tobytes() and info[i, 1] > 0
        assert np.array_equal(probs[i], A.default_probs())


def test_baselines_per_job_and_one_for_all(contexts, restated):
    """probs_in: a set per job, all different, and one set with stride 0"""
    ctx = contexts((48, 32))
    jobs = [content(2, 3, f, l, 60 + k) for k, (f, l) in enumerate((("alphabet", "sparse"), ("far", "dense"), ("alphabet", "edges")))]
    sets = np.stack([other_probs(k) for k in range(3)])
    got = pack(ctx, jobs, probs_in=sets, refresh_entropy_probs=0)
    for i, job in enumerate(jobs):
        same(got, i, restated(("per job", i), *job, probs_in=sets[i], refresh_entropy_probs=0), ("per job", i))
    got = pack(ctx, jobs, probs_in=sets[2], flags=A.MV | A.SKIP)
    for i, job in enumerate(jobs):
        same(got, i, restated(("one set", i), *job, probs_in=sets[2], flags=A.MV | A.SKIP), ("one set", i))
        assert np.array_equal(got[3][i, :1056], sets[2, :1056])                 # no coefficient flag: the baseline stays


@pytest.mark.parametrize("n", (9, 65, 130))
def test_many_jobs_of_different_content(contexts, restated, n):
    """32x32, one partition: neighbouring coder lanes and the workgroups of the count kernel hold different jobs and tables"""
    ctx = contexts((32, 32))
    kinds = [(f, l) for f in ("alphabet", "far", "equal", "zero") for l in ("sparse", "dense", "edges", "zero")]
    jobs = [content(2, 2, *kinds[i % 16], 200 + i) for i in range(n)]
    sets = np.stack([other_probs(1000 + i) if i % 3 else A.default_probs() for i in range(n)])
    got = pack(ctx, jobs, cap=16384, probs_in=sets)
    for i, job in enumerate(jobs):
        same(got, i, restated(("many", i), *job, probs_in=sets[i]), ("many", n, i))


def test_1030_jobs_cross_the_group_limit(contexts, restated):
    ctx = contexts((16, 16))
    kinds = [content(1, 1, f, l, 300 + k) for k, (f, l) in enumerate((("alphabet", "sparse"), ("far", "dense"), ("zero", "zero"), ("equal", "edges"),
                                                                      ("far", "sparse"), ("alphabet", "dense"), ("zero", "edges")))]
    qs = [3 * (i % 10) + 7 for i in range(1030)]
    jobs = [kinds[i % 7] for i in range(1030)]
    got = pack(ctx, jobs, cap=4096, qindex=qs)
    for i in range(1030):
        same(got, i, restated(("1030", i % 7), *jobs[i], qindex=qs[i]), i)


def test_statuses(contexts, restated):
    """a job the plan refuses counts nothing and updates nothing, and its neighbours are untouched; an overflow keeps its counts"""
    ctx = contexts((48, 32))
    mv, lv = content(2, 3, "alphabet", "sparse", 5)
    good = restated(("status", "good"), mv, lv)
    odd = mv.copy(); odd[0, 1, 1] += 1
    big = lv.copy(); big[1, 2, 17, 5] = 2115
    base = other_probs(9)
    jobs = [(mv, lv), (odd, lv), (mv, big), (mv, lv)]
    got = pack(ctx, jobs)
    for i in (0, 3):
        same(got, i, good, i)
    got = pack(ctx, jobs, probs_in=base)
    for i, bit in ((1, R.BAD_VECTOR), (2, R.BAD_LEVEL)):
        want = A.restate(*jobs[i], probs_in=base)
        assert got[1][i, 0] & 7 == bit and got[1][i, 0] == want["status"] and got[1][i, 1] == 0
        assert got[1][i, 11:].tolist() == want["info"][11:].tolist() and not got[2][i].any() and np.array_equal(got[3][i], base)
    n = len(good["data"])
    cap = (n + 15) // 16 * 16
    same(pack(ctx, [(mv, lv)], cap=cap), 0, good, "cap fits")
    got = pack(ctx, [(mv, lv)], cap=cap - 16)
    want = A.restate(mv, lv, cap=cap - 16)
    assert want["status"] & 7 == R.OVERFLOW
    same(got, 0, want, "overflow")


def coded(ctx, fb):
    """the three coded planes of a frame buffer as downloaded"""
    return [np.ascontiguousarray(p) for p in SC.planes(ctx.download_full(fb), ctx.g)]


def test_closure_and_a_chain_of_three_frames(pkg, restated):
    """pictures to bytes without the host, and back: a key frame, then frame A (refresh_last 0, refresh_entropy_probs 1), then
    frame B coded with A's probs_out as its baseline, both predicted from the key frame: frames_motion (d = 4), frames_subpel,
    frames_quant at qindex 40, frames_pack_adapt with all flags.  Parsed and decoded by the product one after the other, A and B
    equal frames_quant's rec byte for byte -- B only because the decoder kept what A updated --, and their bytes are the
    restatement's"""
    P = pkg
    w, h, q = 48, 32, 40
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

        def moved(p, dy, dx):
            return TR.edge(p, dy, dx, p.shape[0], p.shape[1]).astype(np.int64)
        for fb, (dy, dx, seed) in ((5, (2, -1, 5)), (4, (-2, 3, 6))):
            pic = TR.noisy([((moved(p, dy >> (i > 0), dx) + moved(p, dy >> (i > 0), dx - 1) + 1) >> 1).astype(np.uint8) for i, p in enumerate(key)], seed, 2)
            pic[0] = np.clip(pic[0].astype(np.int64) + 4 + np.arange(w) // 8, 0, 255).astype(np.uint8)
            ctx.upload_frame(fb, picture_into(np.random.default_rng(fb).integers(0, 256, ctx.g.frame_size, dtype=np.uint8), ctx.g, pic))
        jobs = [(5, last), (4, last)]
        whole, _ = ctx.frames_motion(jobs, 4, planes=())
        mv, _ = ctx.frames_subpel(jobs, start=whole, planes=())
        got = ctx.frames_quant(jobs, mv, q, filter="sixtap", stage="levels", want=("coef", "rec"))
        probs_in = None
        for k, name in enumerate("AB"):
            fields = dict(qindex=q, filter_level=0, refresh_last=0 if name == "A" else 1)
            data, info, _, probs = ctx.frames_pack_adapt(mv[k:k + 1], got["coef"][k:k + 1], cap=8192, refresh_entropy_probs=1, probs_in=probs_in,
                                                         probs=True, **fields)
            frame = P.pack_frames(data, info)[0]
            info = info.cpu().numpy()
            assert info[0, 0] == 0 and info[0, 16] > 0 and len(frame) == info[0, 1]
            want = A.restate(mv[k].cpu().numpy(), got["coef"][k].cpu().numpy(), probs_in=None if probs_in is None else probs_in.cpu().numpy(), **fields)
            assert frame == want["data"] and info[0].tolist() == want["info"].tolist() and np.array_equal(probs[0].cpu().numpy(), want["probs_out"])
            if probs_in is not None:
                assert not np.array_equal(probs_in.cpu().numpy(), A.default_probs())     # B's baseline is not the default: A updated it
            probs_in = probs[0].clone()
            hdr2 = ctx.parse_into_slot(parser, frame, 0)
            ctx.upload(0)
            r = parser.refs
            assert r.lst_idx == last and r.new_idx not in (4, 5)
            ctx.decode([(0, r.new_idx, (r.lst_idx, r.gld_idx, r.alt_idx))], P.STAGE_ALL)
            ctx.sync()
            decoded = TR.pack(coded(ctx, r.new_idx), w, h)
            rec = got["rec"][k].cpu().numpy()
            assert np.array_equal(decoded, rec), (name, np.flatnonzero(decoded != rec)[:8].tolist())
            assert hdr2.base_qindex == q
            parser.swap(hdr2)
    finally:
        parser.close()
        ctx.close()


def raw_call(ctx, P, n, mv, mv_stride, coef, coef_stride, dst, dst_stride, cap, info, counts, probs_out, flags=15, refresh=1, probs_in=None,
             probs_in_stride=0, null_adapt=False, qindex=40, **fields):
    """vp8hip_frames_pack_adapt_async itself, on pointers: -> its status"""
    p = P.PackParams()
    for name, v in {**P.PACK_DEFAULTS, **fields}.items():
        setattr(p, name, v)
    p.qindex = qindex
    a = P.PackAdapt(flags, refresh, probs_in, probs_in_stride)
    vp = ctypes.c_void_p
    return ctx.L.vp8hip_frames_pack_adapt_async(ctx.h, n, ctypes.byref(p), None if null_adapt else ctypes.byref(a), vp(mv) if mv else None, mv_stride,
                                                vp(coef) if coef else None, coef_stride, vp(dst) if dst else None, dst_stride, cap,
                                                vp(info) if info else None, vp(counts) if counts else None, vp(probs_out) if probs_out else None)


def test_the_wrapper_and_the_refusals(pkg, contexts):
    """shapes and types, optional outputs, what the wrapper and the call refuse"""
    P = pkg
    ctx = contexts((48, 32))
    mv_a, lv_a = content(2, 3, "alphabet", "sparse", 5)
    n = 3
    mv = torch.from_numpy(np.stack([mv_a] * n)).to("cuda:0")
    coef = torch.from_numpy(np.stack([lv_a] * n)).to("cuda:0")
    data, info, counts, probs = ctx.frames_pack_adapt(mv, coef, log2_parts=2)
    bound = ctx.pack_adapt_bound(2)
    assert counts is None and probs is None and tuple(data.shape) == (n, bound) and info.dtype == torch.int32 and tuple(info.shape) == (n, 32)
    data, info, counts, probs = ctx.frames_pack_adapt(mv, coef, log2_parts=2, counts=True, probs=True, cap=2048)
    assert counts.dtype == torch.int32 and tuple(counts.shape) == (n, 1216) and probs.dtype == torch.uint8 and tuple(probs.shape) == (n, 1104)
    want = A.restate(mv_a, lv_a, log2_parts=2)
    assert P.pack_frames(data, info) == [want["data"]] * n and np.array_equal(probs[1].cpu().numpy(), want["probs_out"])
    assert np.array_equal(P.pack_probs_default(), A.default_probs())
    one = torch.from_numpy(other_probs(4)).to("cuda:0")
    for bad in (dict(flags=16), dict(flags=-1), dict(refresh_entropy_probs=2), dict(probs_in=one[:1100]), dict(probs_in=one.cpu()),
                dict(probs_in=one.to(torch.int16)), dict(probs_in=torch.stack([one, one])), dict(cap=100), dict(qindex=128), dict(nonsense=1),
                dict(out_info=torch.zeros((n, 16), dtype=torch.int32, device="cuda:0")), dict(out_counts=torch.zeros((n, 1216), dtype=torch.int64, device="cuda:0")),
                dict(out_probs=torch.zeros((n, 1100), dtype=torch.uint8, device="cuda:0"))):
        with pytest.raises((ValueError, RuntimeError)):
            ctx.frames_pack_adapt(mv, coef, **bad)
    # the call itself, on pointers
    cap, msize, csize = 1024, 4 * 6, 800 * 6
    dst = torch.full((8 * cap,), 0xA5, dtype=torch.uint8, device="cuda:0")
    inf = torch.full((8 * 32,), -1, dtype=torch.int32, device="cuda:0")
    cnt = torch.full((8 * 1216,), -1, dtype=torch.int32, device="cuda:0")
    pout = torch.full((8 * 1104,), 0xA5, dtype=torch.uint8, device="cuda:0")
    pin = torch.from_numpy(np.stack([other_probs(k) for k in range(8)])).to("cuda:0")
    mv, coef = torch.from_numpy(np.stack([mv_a] * 8)).to("cuda:0"), torch.from_numpy(np.stack([lv_a] * 8)).to("cuda:0")     # (every buffer holds eight jobs)
    ok = dict(n=n, mv=mv.data_ptr(), mv_stride=msize, coef=coef.data_ptr(), coef_stride=csize, dst=dst.data_ptr(), dst_stride=cap, cap=cap,
              info=inf.data_ptr(), counts=cnt.data_ptr(), probs_out=pout.data_ptr(), probs_in=pin.data_ptr(), probs_in_stride=1104)

    def call(**kw):
        return raw_call(ctx, P, **{**ok, **kw})
    assert call() == 0 and call(counts=None, probs_out=None, probs_in=None) == 0 and call(probs_in_stride=0) == 0 and call(probs_in_stride=2208) == 0
    ctx.sync()
    filled = [t.clone() for t in (dst, inf, cnt, pout)]
    assert_destinations_refused(ctx, lambda k, d, s: call(n=k, dst=d, dst_stride=s), dst.data_ptr(), cap, 16)
    assert_destinations_refused(ctx, lambda k, d, s: call(n=k, coef=d, coef_stride=s), coef.data_ptr(), csize, 16)
    assert_destinations_refused(ctx, lambda k, d, s: call(n=k, probs_in=d, probs_in_stride=s), pin.data_ptr(), 1104, 16, null=False)
    assert call(null_adapt=True) == -2 and call(flags=16) == -2 and call(flags=-1) == -2 and call(refresh=2) == -2 and call(refresh=-1) == -2
    assert call(info=None) == -2 and call(info=inf.data_ptr() + 2) == -2 and call(info=np.zeros(128, np.int32).ctypes.data) == -2
    assert call(counts=cnt.data_ptr() + 2) == -2 and call(counts=np.zeros(8 * 1216, np.int32).ctypes.data) == -2
    assert call(probs_out=pout.data_ptr() + 8) == -2 and call(probs_out=np.zeros(8 * 1104, np.uint8).ctypes.data) == -2
    assert call(probs_in=pin.data_ptr() + 8) == -2 and call(probs_in_stride=1088) == -2 and call(probs_in_stride=1112) == -2
    assert call(n=9) == -2                                                      # every buffer holds eight jobs
    assert call(n=0) == -2 and call(cap=cap + 16) == -2 and call(cap=8) == -2
    assert call(info=dst.data_ptr()) == -2 and call(counts=inf.data_ptr()) == -2 and call(probs_out=dst.data_ptr()) == -2
    assert call(probs_out=pin.data_ptr()) == -2 and call(counts=coef.data_ptr()) == -2 and call(info=mv.data_ptr()) == -2
    for bad in (dict(qindex=128), dict(version=4), dict(ref_frame=0), dict(log2_parts=4), dict(prob_skip_false=0), dict(prob_gf=256)):
        assert call(**bad) == -2, bad
    ctx.sync()
    assert all(torch.equal(t, f) for t, f in zip((dst, inf, cnt, pout), filled))   # nothing was enqueued by any of them
    assert b"vp8hip_frames_pack_adapt_async" in ctx.L.vp8hip_last_error(ctx.h)
