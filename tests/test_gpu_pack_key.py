"""GPU (-m gpu): compressed VP8 key frames from intra modes and levels in device memory (vp8hip_frames_pack_key_async;
Vp8Hip.frames_pack_key; csrc/hip/vp8_pack_key.hip), byte for byte and info entry for entry against the restatement
(tests/pack_key_reference.py: the stream writer of tests/vp8_writer.py, which tests/test_pack_key_cpu.py holds to the real reference
decoder).  The closure tests make a two-frame stream whose every byte came from the device -- frames_intra and frames_pack_key,
then frames_motion, frames_subpel, frames_quant and frames_pack -- and decode it with the product's own decoder to the encoder's
reconstructions.  torch is imported here, before the package loads libvpx's library: one HIP runtime per process."""
import ctypes

import torch  # noqa: F401  (first: the library then shares torch's HIP runtime)
import numpy as np
import pytest

from handover_testlib import assert_destinations_refused, assert_guards_intact, guarded, picture_into
import intra_reference as IR
import pack_key_reference as K
import pack_reference as R
import scale_reference as SC
import tfilter_reference as TR

pytestmark = pytest.mark.gpu

KINDS = ("bpred", "16x16", "mixed")
LEVELS = ("zero", "sparse", "dense", "edges")


@pytest.fixture(scope="module")
def contexts(pkg):
    """one context of six frame buffers per display size, shared by the tests of this module"""
    made = {}

    def get(size):
        if size not in made:
            ctx = pkg.Vp8Hip(0)
            ctx.configure(size[0], size[1], 6, 1)
            made[size] = ctx
        return made[size]
    yield get
    for ctx in made.values():
        ctx.close()


@pytest.fixture(scope="module")
def restated():
    """the restatement of (content key, parameters), computed once"""
    memo = {}

    def get(key, modes, lv, **kw):
        k = (key, tuple(sorted(kw.items())))
        if k not in memo:
            memo[k] = K.restate(modes, lv, **kw)
        return memo[k]
    return get


def content(rows, cols, kind, levels, seed):
    return K.make_modes(kind, rows, cols, seed), K.make_levels(levels, rows, cols, seed)


def pack(ctx, jobs, cap=None, pad=48, qindex=40, strided=False, **fields):
    """frames_pack_key over jobs = [(modes, levels)] into guarded memory -> (data, info) as arrays; the guards round every job's
    frame and round the info are checked.  strided: strides larger than the sizes, other bytes between the jobs' modes and levels"""
    n = len(jobs)
    rows, cols = jobs[0][1].shape[:2]
    cap = ctx.pack_key_bound(fields.get("log2_parts", 0)) if cap is None else cap
    big, data = guarded(n, cap, pad, 64)
    ibig = torch.full(((n + 2) * 16,), -1515870811, dtype=torch.int32, device="cuda:0")      # 0xA5A5A5A5
    out_info = ibig[16:16 + 16 * n].view(n, 16)
    lv = np.stack([j[1] for j in jobs]).astype(np.int16)
    md = np.stack([j[0] for j in jobs]).astype(np.uint8)
    if strided:
        wide = torch.full((n, lv[0].size + 24), 0x5A5A, dtype=torch.int16, device="cuda:0")
        wide[:, :lv[0].size] = torch.from_numpy(lv.reshape(n, -1)).to("cuda:0")
        coef = wide.as_strided((n, rows, cols, 25, 16), (lv[0].size + 24, cols * 400, 400, 16, 1))
        mwide = torch.full((n, md[0].size + 12), 0xA5, dtype=torch.uint8, device="cuda:0")
        mwide[:, :md[0].size] = torch.from_numpy(md.reshape(n, -1)).to("cuda:0")
        modes = mwide.as_strided((n, rows, cols, 32), (md[0].size + 12, cols * 32, 32, 1))
    else:
        coef = torch.from_numpy(lv).to("cuda:0")
        modes = torch.from_numpy(md).to("cuda:0")
    d, info = ctx.frames_pack_key(modes, coef, qindex=qindex, cap=cap, out_data=data, out_info=out_info, **fields)
    assert d is data and info is out_info
    torch.cuda.synchronize()
    assert_guards_intact(big, n, cap, pad, 64, what="bytes outside the jobs' regions were written")
    edge = ibig.cpu().numpy()
    assert (edge[:16] == -1515870811).all() and (edge[16 + 16 * n:] == -1515870811).all(), "words outside the jobs' info were written"
    if strided:
        assert (mwide[:, md[0].size:] == 0xA5).all() and (wide[:, lv[0].size:] == 0x5A5A).all()
    return data.cpu().numpy(), info.cpu().numpy().astype(np.int64)


def same(data, info, i, want, what):
    """job i of pack() against a restatement"""
    assert info[i].tolist() == want["info"].tolist(), (what, i, info[i].tolist(), want["info"].tolist())
    if want["data"] is not None:
        got = data[i, :info[i, 1]].tobytes()
        bad = [k for k in range(min(len(got), len(want["data"]))) if got[k] != want["data"][k]][:8]
        assert got == want["data"], (what, i, len(got), len(want["data"]), bad)


@pytest.mark.parametrize("lp", range(4))
def test_48x32_every_kind_of_modes_and_content(contexts, restated, lp):
    """3 kinds of modes x 4 kinds of levels in one call, at 1, 2, 4 and 8 partitions (two rows: six of the eight are empty)"""
    ctx = contexts((48, 32))
    keys = [(k, l) for k in KINDS for l in LEVELS]
    jobs = [content(2, 3, k, l, 11 + i) for i, (k, l) in enumerate(keys)]
    data, info = pack(ctx, jobs, log2_parts=lp)
    for i, ((k, l), (modes, lv)) in enumerate(zip(keys, jobs)):
        want = restated(("48x32", k, l, i), modes, lv, log2_parts=lp)
        same(data, info, i, want, (k, l, lp))
        assert info[i, 0] == 0 and (info[i, 13:] == 0).all()
        assert (info[i, 3 + (1 << lp):11] == 0).all() and (info[i, 3:3 + (1 << lp)] >= 4).all()
        if lp == 3:
            assert (info[i, 5:11] == 4).all()                                   # an empty partition is its flush
        if l == "zero":
            assert info[i, 11] == 6 and (info[i, 3:3 + (1 << lp)] == 4).all()   # every macroblock skipped
        assert info[i, 12] == (6 if k == "bpred" else 0 if k == "16x16" else (modes[..., 0] == 4).sum())


def named_content(name):
    """(size, display, [(modes, levels)]) of the cases the CPU test holds to the reference decoder, and of 176x144"""
    if name == "cover":
        modes = K.make_cover_modes(4, 4, 0)
        assert len(K.coverage(modes)[3]) == 100
        return (64, 64), (64, 64), [(modes, K.make_levels(l, 4, 4, 0)) for l in ("sparse", "edges")]
    if name == "y2":
        return (64, 64), (64, 64), [K.y2_context_case(has, column) for column in (True, False) for has in (True, False)]
    if name == "odd":
        return (80, 48), (67, 45), [content(3, 5, k, l, 9) for k, l in (("mixed", "sparse"), ("bpred", "edges"), ("16x16", "dense"))]
    if name == "one":
        return (16, 16), (16, 16), [content(1, 1, k, l, 40 + i) for i, (k, l) in enumerate([(k, l) for k in KINDS[:2] for l in LEVELS])]
    assert name == "qcif"
    return (176, 144), (176, 144), [content(9, 11, k, "dense", 31 + i) for i, k in enumerate(KINDS)]


@pytest.mark.parametrize("name,lp", [("one", 0), ("one", 3), ("cover", 0), ("y2", 0), ("y2", 1), ("odd", 3), ("qcif", 3), ("qcif", 0)])
def test_other_sizes(pkg, contexts, restated, name, lp):
    """16x16 (one macroblock: every neighbour outside), the frame with every mode and context pair, the Y2-context cases, 80x48 shown
    as 67x45 with 8 partitions and padded strides, 176x144 dense all-B_PRED, no-B_PRED and mixed"""
    size, display, jobs = named_content(name)
    ctx = contexts(display)
    data, info = pack(ctx, jobs, log2_parts=lp, strided=display != size)
    for i, (modes, lv) in enumerate(jobs):
        same(data, info, i, restated((name, i), modes, lv, log2_parts=lp, display=display), (name, lp))
    if name == "y2":
        assert data[0, :info[0, 1]].tobytes() != data[1, :info[1, 1]].tobytes() and info[:, 12].tolist() == [2] * 4
    if name == "odd":
        assert data[0, 6:10].tobytes() == bytes([67, 0, 45, 0])
    assert ctx.pack_key_bound(lp) == pkg.pack_key_bound(display[0], display[1], lp)


def test_every_magnitude_at_which_the_tokens_change(contexts, restated):
    """both signs of every magnitude at which the token tree or a DCT category changes, at luma position 0 of B_PRED blocks and at
    the other steps"""
    ctx = contexts((16, 16))
    modes = K.make_modes("bpred", 1, 1, 3)
    jobs = []
    for sign in (1, -1):
        for pos in (0, 1, 15):
            lv = np.zeros((1, 1, 25, 16), np.int16)
            lv[0, 0, :16, pos] = sign * np.array(R.CAT_EDGES)
            lv[0, 0, 16:24, pos] = -sign * np.array(R.CAT_EDGES[8:])
            jobs.append((modes, lv))
    data, info = pack(ctx, jobs)
    for i, (m, lv) in enumerate(jobs):
        want = restated(("magnitudes", i), m, lv)
        assert want["status"] == 0 and want["info"][11] == 0
        same(data, info, i, want, i)


def test_what_is_not_read_changes_no_byte(contexts, restated):
    """luma position 0 and the sub-block modes of 16x16 macroblocks, block 24 of B_PRED macroblocks, modes[2], [3] and [20..31]: set
    to anything, 255 and levels beyond DCT_CAT6 included, they change no byte and set no status"""
    ctx = contexts((48, 32))
    modes, lv = content(2, 3, "mixed", "sparse", 5)
    modes[0, 0, 0], modes[0, 1, 0], modes[1, 2, 0] = K.B_PRED, 1, 3
    bpred = modes[..., 0] == K.B_PRED
    rng = np.random.default_rng(3)
    noisy = lv.copy()
    noisy[~bpred, :16, 0] = rng.integers(-32768, 32768, size=((~bpred).sum(), 16))
    noisy[bpred, 24] = rng.integers(-32768, 32768, size=(bpred.sum(), 16))
    other = modes.copy()
    other[..., 2:4], other[..., 20:] = rng.integers(0, 256, size=(2, 3, 2)), 255
    other[~bpred, 4:20] = 255
    blank = np.zeros_like(lv)
    blank[~bpred, :16, 0], blank[bpred, 24] = 2115, -2115      # ... not even where nothing else is coded: the macroblocks are skipped
    data, info = pack(ctx, [(modes, lv), (modes, noisy), (other, lv), (other, noisy), (other, blank)])
    want = restated(("unread", 0), modes, lv)
    for i in range(4):
        same(data, info, i, want, i)
    assert info[4, 0] == 0 and info[4, 11] == 6 and info[4, 12] == bpred.sum()
    same(data, info, 4, restated(("unread", 4), modes, np.zeros_like(lv)), "skipped")


def test_130_different_jobs_in_neighbouring_lanes(contexts, restated):
    """130 different jobs: three workgroups of first-partition lanes, and with 2 partitions five of token lanes"""
    ctx = contexts((48, 32))
    jobs = [content(2, 3, KINDS[i % 3], LEVELS[1 + i % 3], 200 + i) for i in range(130)]
    data, info = pack(ctx, jobs, cap=8192, log2_parts=1, prob_skip_false=90)
    assert len({data[i, :info[i, 1]].tobytes() for i in range(130)}) == 130
    for i, (modes, lv) in enumerate(jobs):
        same(data, info, i, restated(("130", i), modes, lv, log2_parts=1, prob_skip_false=90), i)


def test_1030_jobs_of_ten_qindex_values(contexts, restated):
    """1030 jobs cross the launch's job table and, with ten qindex values, its header table; strides larger than the sizes"""
    ctx = contexts((48, 32))
    kinds = [content(2, 3, KINDS[k % 3], LEVELS[(k // 2) % 4], 70 + k) for k in range(8)]
    qs = [3 * (i % 10) + 7 for i in range(1030)]
    jobs = [kinds[i % 8] for i in range(1030)]
    fields = dict(log2_parts=1, version=2, show_frame=0, color_space=1, clamping_type=1, filter_type=1, filter_level=33, sharpness=5)
    data, info = pack(ctx, jobs, cap=8192, qindex=qs, strided=True, deltas=(1, -2, 3, -4, 5), **fields)
    for i in range(1030):
        same(data, info, i, restated(("many", i % 8), *jobs[i], qindex=qs[i], deltas=(1, -2, 3, -4, 5), **fields), i)
    data, info = pack(ctx, jobs[5:6], cap=8192)
    same(data, info, 0, restated(("one", 5), *jobs[5]), "one job")


def test_1920x1080_with_sparse_levels(contexts, restated):
    """one job of 8160 macroblocks with mixed modes, 8 partitions; levels in one block of twenty, so that the restatement stays quick"""
    ctx = contexts((1920, 1080))
    rng = np.random.default_rng(8)
    modes = K.make_modes("mixed", 68, 120, 8)
    lv = np.zeros((68, 120, 25, 16), np.int16)
    hit = rng.random((68, 120, 25)) < 0.05
    lv[..., :3][hit] = rng.integers(-6, 7, size=(int(hit.sum()), 3))
    data, info = pack(ctx, [(modes, lv)], cap=1 << 20, log2_parts=3, qindex=10)
    want = restated(("1080p", 0), modes, lv, log2_parts=3, qindex=10, display=(1920, 1080))
    assert 1000 < want["info"][11] < 7000 and 2000 < want["info"][12] < 6000
    same(data, info, 0, want, "1080p")


def test_statuses(contexts, restated):
    """BAD_MODE by each of its three causes, BAD_LEVEL, OVERFLOW with the sizes that would have fitted; a failing job's frame
    bytes are 0 and its neighbours in the call are untouched"""
    ctx = contexts((48, 32))
    modes, lv = content(2, 3, "mixed", "sparse", 5)
    modes[0, 0, 0], modes[1, 2, 0] = K.B_PRED, 2
    good = restated(("status", "good"), modes, lv)

    def with_mode(at, v):
        m = modes.copy()
        m[at] = v
        return m
    ybad, uvbad, subbad = with_mode((1, 1, 0), 5), with_mode((0, 2, 1), 4), with_mode((0, 0, 9), 10)
    ymax, submax = with_mode((1, 1, 0), 255), with_mode((0, 0, 19), 255)
    big = lv.copy(); big[1, 2, 17, 5] = 2115
    pos0 = lv.copy(); pos0[0, 0, 3, 0] = -2115                          # luma position 0 of a B_PRED macroblock is coded
    top = lv.copy(); top[0, 0, 3, 0] = -2114
    jobs = [(modes, lv), (ybad, lv), (modes, lv), (uvbad, lv), (subbad, lv), (modes, big), (modes, pos0), (modes, top), (ymax, big), (submax, lv),
            (modes, lv)]
    data, info = pack(ctx, jobs)
    for i in (0, 2, 10):
        same(data, info, i, good, i)
    for i, bit in ((1, K.BAD_MODE), (3, K.BAD_MODE), (4, K.BAD_MODE), (5, K.BAD_LEVEL), (6, K.BAD_LEVEL), (8, K.BAD_MODE | K.BAD_LEVEL), (9, K.BAD_MODE)):
        want = K.restate(*jobs[i])
        assert info[i, 0] == bit == want["status"] and info[i, 1] == 0, (i, info[i].tolist())
        assert info[i, 11:].tolist() == want["info"][11:].tolist(), (i, info[i].tolist())
    same(data, info, 7, K.restate(modes, top), "a level of -2114 at luma position 0")
    # cap: the frame rounded up fits; 16 less and it alone overflows
    small = content(2, 3, "16x16", "zero", 1)
    n = len(good["data"])
    cap = (n + 15) // 16 * 16
    data, info = pack(ctx, [small, (modes, lv), small], cap=cap)
    same(data, info, 1, good, "cap fits")
    data, info = pack(ctx, [small, (modes, lv), small], cap=cap - 16)
    assert info[1, 0] == K.OVERFLOW and info[1, 1] == 0 and info[1, 2:].tolist() == good["info"][2:].tolist()
    assert 10 + info[1, 2] + info[1, 3:11].sum() == n
    for i in (0, 2):
        same(data, info, i, K.restate(*small), "beside an overflow")
    data, info = pack(ctx, [(modes, lv)], cap=16)
    assert info[0, 0] == K.OVERFLOW and info[0, 1] == 0


def test_two_calls_without_a_sync(contexts, restated):
    """the second call's scratch is the first one's: the stream orders them"""
    ctx = contexts((48, 32))
    a, b = content(2, 3, "mixed", "dense", 1), content(2, 3, "bpred", "edges", 2)
    ta = [torch.from_numpy(np.stack([x] * 3)).to("cuda:0") for x in a]
    tb = [torch.from_numpy(np.stack([x] * 70)).to("cuda:0") for x in b]
    da, ia = ctx.frames_pack_key(*ta, cap=8192, log2_parts=2)
    db, ib = ctx.frames_pack_key(*tb, cap=8192)
    torch.cuda.synchronize()
    wa, wb = restated(("two", "a"), *a, log2_parts=2), restated(("two", "b"), *b)
    for d, i, want, n in ((da, ia, wa, 3), (db, ib, wb, 70)):
        d, i = d.cpu().numpy(), i.cpu().numpy().astype(np.int64)
        for k in range(n):
            same(d, i, k, want, k)


def raw_call(ctx, P, n, modes, modes_stride, coef, coef_stride, dst, dst_stride, cap, info, qindex=40, jq=None, **fields):
    """vp8hip_frames_pack_key_async itself, on pointers: -> its status"""
    p = P.PackKeyParams()
    for name, v in {**P.PACK_KEY_DEFAULTS, **fields}.items():
        setattr(p, name, v)
    p.qindex = qindex
    keep = None if jq is None else (ctypes.c_uint8 * len(jq))(*jq)
    if keep is not None:
        p.job_qindex = keep
    vp = ctypes.c_void_p
    return ctx.L.vp8hip_frames_pack_key_async(ctx.h, n, ctypes.byref(p), vp(modes) if modes else None, modes_stride, vp(coef) if coef else None,
                                              coef_stride, vp(dst) if dst else None, dst_stride, cap, vp(info) if info else None)


def test_the_wrapper_and_the_refusals(pkg, contexts):
    """shapes and types, out_* filled and returned, pack_frames, what the wrapper and the call refuse"""
    P = pkg
    ctx = contexts((48, 32))
    md_a, lv_a = content(2, 3, "mixed", "sparse", 5)
    n = 3
    bad_md = md_a.copy(); bad_md[0, 0, 1] = 4
    modes = torch.from_numpy(np.stack([md_a, bad_md, md_a])).to("cuda:0")
    coef = torch.from_numpy(np.stack([lv_a] * n)).to("cuda:0")
    bound = ctx.pack_key_bound(2)
    assert bound == P.pack_key_bound(48, 32, 2) and bound % 16 == 0 and P.PACK_BAD_MODE == 16
    data, info = ctx.frames_pack_key(modes, coef, log2_parts=2)
    assert data.dtype == torch.uint8 and tuple(data.shape) == (n, bound) and info.dtype == torch.int32 and tuple(info.shape) == (n, 16)
    frames = P.pack_frames(data, info)
    want = K.restate(md_a, lv_a, log2_parts=2)["data"]
    assert frames[0] == frames[2] == want and frames[1] is None and int(info[1, 0]) == P.PACK_BAD_MODE
    out_data = torch.zeros((n, 1024), dtype=torch.uint8, device="cuda:0")
    out_info = torch.zeros((n, 16), dtype=torch.int32, device="cuda:0")
    d2, i2 = ctx.frames_pack_key(modes, coef, log2_parts=2, out_data=out_data, out_info=out_info)
    assert d2 is out_data and i2 is out_info and torch.equal(i2, info) and P.pack_frames(d2, i2) == frames
    for bad in (dict(qindex=128), dict(qindex=[40, 40]), dict(qindex=[40, 40, 200]), dict(deltas=(0, 0, 0, 0, 16)), dict(log2_parts=4),
                dict(prob_skip_false=0), dict(prob_skip_false=256), dict(cap=100), dict(cap=0), dict(nonsense=1), dict(ref_frame=1), dict(filter_level=64),
                dict(version=4), dict(color_space=2), dict(clamping_type=-1),
                dict(out_data=torch.zeros((n, 1024), dtype=torch.int8, device="cuda:0")), dict(out_info=torch.zeros((n, 8), dtype=torch.int32, device="cuda:0")),
                dict(out_data=torch.zeros((n + 1, 1024), dtype=torch.uint8, device="cuda:0")), dict(out_data=torch.zeros((n, 1024), dtype=torch.uint8))):
        with pytest.raises((ValueError, RuntimeError)):
            ctx.frames_pack_key(modes, coef, **bad)
    for bad_modes, bad_coef in ((modes[:2], coef), (modes.to(torch.int8), coef), (modes, coef.to(torch.int32)), (modes, coef[:, :1]), (modes[:, :1], coef),
                                (modes.cpu(), coef), (modes, coef.cpu()), (None, coef)):
        with pytest.raises(ValueError):
            ctx.frames_pack_key(bad_modes, bad_coef)
    # the call itself, on pointers
    cap, msize, csize = 1024, 32 * 6, 800 * 6
    dst = torch.full((8 * cap,), 0xA5, dtype=torch.uint8, device="cuda:0")
    inf = torch.full((8 * 16,), -1, dtype=torch.int32, device="cuda:0")
    spare = torch.zeros((8 * msize,), dtype=torch.uint8, device="cuda:0")      # modes with room behind them for the destinations' tests
    spare[:n * msize] = modes.reshape(-1)
    ok = dict(n=n, modes=spare.data_ptr(), modes_stride=msize, coef=coef.data_ptr(), coef_stride=csize, dst=dst.data_ptr(), dst_stride=cap, cap=cap,
              info=inf.data_ptr())

    def call(**kw):
        return raw_call(ctx, P, **{**ok, **kw})
    assert call() == 0
    ctx.sync()
    filled = (dst.clone(), inf.clone())
    assert_destinations_refused(ctx, lambda k, d, s: call(n=k, dst=d, dst_stride=s), dst.data_ptr(), cap, 16)
    assert_destinations_refused(ctx, lambda k, d, s: call(n=k, coef=d, coef_stride=s), coef.data_ptr(), csize, 16)
    assert_destinations_refused(ctx, lambda k, d, s: call(n=k, modes=d, modes_stride=s), spare.data_ptr(), msize, 4)
    assert call(info=None) == -2 and call(info=inf.data_ptr() + 2) == -2 and call(info=np.zeros(64, np.int32).ctypes.data) == -2
    assert call(n=0) == -2 and call(n=-1) == -2
    assert call(cap=cap + 16) == -2 and call(cap=cap - 8) == -2 and call(cap=0) == -2 and call(cap=8) == -2
    assert call(dst=coef.data_ptr(), dst_stride=csize) == -2 and call(info=dst.data_ptr()) == -2 and call(dst=spare.data_ptr(), cap=16, dst_stride=16) == -2
    assert call(info=coef.data_ptr()) == -2 and call(info=spare.data_ptr()) == -2
    for bad in (dict(qindex=-1), dict(qindex=128), dict(jq=[1, 2, 128]), dict(version=4), dict(version=-1), dict(show_frame=2), dict(color_space=2),
                dict(clamping_type=2), dict(filter_type=-1), dict(filter_level=64), dict(sharpness=8), dict(log2_parts=4), dict(log2_parts=-1),
                dict(prob_skip_false=0), dict(prob_skip_false=256)):
        assert call(**bad) == -2, bad
    ctx.sync()
    assert torch.equal(dst, filled[0]) and torch.equal(inf, filled[1])         # nothing was enqueued by any of them
    assert b"vp8hip_frames_pack_key_async" in ctx.L.vp8hip_last_error(ctx.h)


def coded(ctx, fb):
    """the three coded planes of a frame buffer as downloaded"""
    return [np.ascontiguousarray(p) for p in SC.planes(ctx.download_full(fb), ctx.g)]


def upload(ctx, fb, planes, rng):
    ctx.upload_frame(fb, picture_into(rng.integers(0, 256, ctx.g.frame_size, dtype=np.uint8), ctx.g, planes))


@pytest.mark.parametrize("w,h,lp,seed,flat", [(48, 32, 0, 61, [(1, 2)]), (176, 144, 3, 8, [(0, 0), (3, 4), (3, 5), (8, 10)])], ids=("48x32", "176x144_8_partitions"))
def test_closure_every_byte_from_the_device(pkg, w, h, lp, seed, flat):
    """frames_intra (bmode_last 9; the picture has flat macroblocks, so a 16x16 mode occurs beside B_PRED) -> frames_pack_key with
    filter level 0 -> parsed and decoded by this library -> equals frames_intra's rec byte for byte, and the frame is the
    restatement's; then frames_motion, frames_subpel, frames_quant, frames_pack of a second picture against that decoded key
    frame decode to frames_quant's rec.  No host writer anywhere in the chain."""
    P = pkg
    q = 40
    ctx = P.Vp8Hip(0)
    parser = P.Parser()
    try:
        ctx.configure(w, h, 6, 1)
        first = [p.copy() for p in IR.picture("decoded", w, h, seed)]
        for r, c in flat:
            for i, p in enumerate(first):
                s = 16 >> (i > 0)
                p[s * r:s * r + s, s * c:s * c + s] = 97
        upload(ctx, 4, first, np.random.default_rng(2))
        got = ctx.frames_intra([4], q, bmode_last=9, want=("coef", "modes", "rec"))
        data, info = ctx.frames_pack_key(got["modes"], got["coef"], qindex=q, filter_level=0, log2_parts=lp, cap=1 << 17)
        key_frame = P.pack_frames(data, info)[0]
        info = info.cpu().numpy().astype(np.int64)
        modes, levels = got["modes"][0].cpu().numpy(), got["coef"][0].cpu().numpy()
        nmb = modes.shape[0] * modes.shape[1]
        assert info[0, 0] == 0 and 0 < info[0, 12] < nmb and info[0, 12] == (modes[..., 0] == 4).sum() and len(key_frame) == info[0, 1]
        want = K.restate(modes, levels, qindex=q, filter_level=0, log2_parts=lp)
        assert key_frame == want["data"] and info[0].tolist() == want["info"].tolist()
        assert info[0, 11] == modes[..., 2].sum()                                # the derived skip flags are frames_intra's
        hdr = ctx.parse_into_slot(parser, key_frame, 0)
        ctx.upload(0)
        r = parser.refs
        assert r.new_idx not in (4, 5) and hdr.frame_type == 0 and (hdr.width, hdr.height) == (w, h)
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
        data2, info2 = ctx.frames_pack(mv, qo["coef"], qindex=q, filter_level=0, log2_parts=lp, cap=1 << 17)
        frames = P.pack_frames(data2, info2)
        assert int(info2[0, 0]) == 0 and len(frames[0]) == int(info2[0, 1])
        hdr2 = ctx.parse_into_slot(parser, frames[0], 0)
        ctx.upload(0)
        r = parser.refs
        assert r.lst_idx == last and r.new_idx not in (4, 5)
        ctx.decode([(0, r.new_idx, (r.lst_idx, r.gld_idx, r.alt_idx))], P.STAGE_ALL)
        ctx.sync()
        decoded = TR.pack(coded(ctx, r.new_idx), w, h)
        rec2 = qo["rec"][0].cpu().numpy()
        assert np.array_equal(decoded, rec2), np.flatnonzero(decoded != rec2)[:8].tolist()
        assert hdr2.base_qindex == q and hdr2.frame_type == 1
    finally:
        parser.close()
        ctx.close()
