"""GPU (-m gpu): compressed VP8 inter frames from quantised levels and vectors in device memory (vp8hip_frames_pack_async;
Vp8Hip.frames_pack; csrc/hip/vp8_pack.hip), byte for byte against the restatement (tests/pack_reference.py: the stream writer of
tests/vp8_writer.py behind the call's mode rule, which tests/test_pack_cpu.py holds to the real reference decoder).  The closure
test puts the call behind frames_motion, frames_subpel and frames_quant and decodes its frame with the product's own decoder.
torch is imported here, before the package loads libvpx's library: one HIP runtime per process."""
import ctypes

import torch  # noqa: F401  (first: the library then shares torch's HIP runtime)
import numpy as np
import pytest

from handover_testlib import assert_destinations_refused, assert_guards_intact, guarded, hip_range, picture_into
import pack_reference as R
import scale_reference as SC
import tfilter_reference as TR
from vp8_testlib import synth_ir
from vp8_writer import write_key_frame

pytestmark = pytest.mark.gpu

FIELDS = ("zero", "equal", "alphabet", "far")
LEVELS = ("zero", "sparse", "dense", "edges")


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
    """the restatement of (content key, parameters), computed once; content() makes the vectors and levels of a key"""
    memo = {}

    def get(key, mv, lv, **kw):
        k = (key, tuple(sorted(kw.items())))
        if k not in memo:
            memo[k] = R.restate(mv, lv, **kw)
        return memo[k]
    return get


def content(rows, cols, field, levels, seed):
    return R.make_field(field, rows, cols, seed), R.make_levels(levels, rows, cols, seed)


def pack(ctx, jobs, cap=None, pad=48, qindex=40, strided=False, **fields):
    """frames_pack over jobs = [(mv or None, levels)] into guarded memory -> (data, info) as arrays; the guards are checked"""
    n = len(jobs)
    rows, cols = jobs[0][1].shape[:2]
    cap = ctx.pack_bound(fields.get("log2_parts", 0)) if cap is None else cap
    big, data = guarded(n, cap, pad, 64)
    lv = np.stack([j[1] for j in jobs]).astype(np.int16)
    if all(j[0] is None for j in jobs):
        mv = None
    else:
        mv = np.stack([np.zeros((2, rows, cols), np.int16) if j[0] is None else j[0] for j in jobs]).astype(np.int16)
    if strided:                                     # strides larger than the sizes, other bytes between the jobs
        wide = torch.full((n, lv[0].size + 24), 0x5A5A, dtype=torch.int16, device="cuda:0")
        wide[:, :lv[0].size] = torch.from_numpy(lv.reshape(n, -1)).to("cuda:0")
        coef = wide.as_strided((n, rows, cols, 25, 16), (lv[0].size + 24, cols * 400, 400, 16, 1))
        if mv is not None:
            mwide = torch.full((n, mv[0].size + 3), 0x5A5A, dtype=torch.int16, device="cuda:0")
            mwide[:, :mv[0].size] = torch.from_numpy(mv.reshape(n, -1)).to("cuda:0")
            mvt = mwide.as_strided((n, 2, rows, cols), (mv[0].size + 3, rows * cols, cols, 1))
    else:
        coef = torch.from_numpy(lv).to("cuda:0")
        mvt = None if mv is None else torch.from_numpy(mv).to("cuda:0")
    if mv is None:
        mvt = None
    d, info = ctx.frames_pack(mvt, coef, qindex=qindex, cap=cap, out_data=data, **fields)
    assert d is data
    torch.cuda.synchronize()
    assert_guards_intact(big, n, cap, pad, 64, what="bytes outside the jobs' regions were written")
    return data.cpu().numpy(), info.cpu().numpy().astype(np.int64)


def same(data, info, i, want, what):
    """job i of pack() against a restatement"""
    assert info[i].tolist() == want["info"].tolist(), (what, i, info[i].tolist(), want["info"].tolist())
    if want["data"] is not None:
        got = data[i, :info[i, 1]].tobytes()
        bad = [k for k in range(len(got)) if got[k] != want["data"][k]][:8]
        assert got == want["data"], (what, i, len(got), bad)


@pytest.mark.parametrize("lp", range(4))
def test_48x32_every_field_and_content(contexts, restated, lp):
    """4 vector fields x 4 kinds of levels in one call, at 1, 2, 4 and 8 partitions (two rows: six of the eight are empty)"""
    ctx = contexts((48, 32))
    keys = [(f, l) for f in FIELDS for l in LEVELS]
    jobs = [content(2, 3, f, l, 11 + k) for k, (f, l) in enumerate(keys)]
    data, info = pack(ctx, jobs, log2_parts=lp)
    modes = np.zeros(4, np.int64)
    for i, ((f, l), (mv, lv)) in enumerate(zip(keys, jobs)):
        want = restated(("48x32", f, l, i), mv, lv, log2_parts=lp)
        same(data, info, i, want, (f, l, lp))
        assert info[i, 0] & 7 == 0 and (info[i, 0] & R.CLAMPS if f == "far" else f == "alphabet" or not info[i, 0])
        assert (info[i, 3 + (1 << lp):11] == 0).all() and (info[i, 3:3 + (1 << lp)] >= 4).all()
        if lp == 3:
            assert (info[i, 5:11] == 4).all()                                   # an empty partition is its flush
        if l == "zero":
            assert info[i, 11] == 6 and (info[i, 3:3 + (1 << lp)] == 4).all()   # every macroblock skipped
        if f == "zero":
            assert info[i, 12] == 6
        if f == "equal":
            assert info[i, 13] == 5 and info[i, 15] == 1                        # NEARESTMV everywhere but the first
        if f == "alphabet":
            modes += info[i, 12:16]
    assert modes.all()


@pytest.mark.parametrize("size,display,lp,keys", [
    ((16, 16), (16, 16), 0, [("alphabet", "dense"), ("zero", "zero"), ("far", "edges"), ("equal", "sparse")]),      # one macroblock: no neighbour at all
    ((16, 16), (16, 16), 3, [("alphabet", "edges"), ("equal", "dense")]),
    ((80, 48), (67, 45), 1, [("alphabet", "sparse"), ("far", "dense"), ("equal", "edges")]),
    ((176, 144), (176, 144), 3, [("alphabet", "dense"), ("equal", "sparse"), ("zero", "zero"), ("far", "edges")]),
    ((176, 144), (176, 144), 0, [("alphabet", "sparse"), ("zero", "dense")]),
], ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_other_sizes(pkg, contexts, restated, size, display, lp, keys):
    ctx = contexts(display)
    rows, cols = size[1] // 16, size[0] // 16
    jobs = [content(rows, cols, f, l, 31 + k) for k, (f, l) in enumerate(keys)]
    data, info = pack(ctx, jobs, log2_parts=lp, strided=display != size)
    for i, ((f, l), (mv, lv)) in enumerate(zip(keys, jobs)):
        same(data, info, i, restated((size, f, l, i), mv, lv, log2_parts=lp), (size, f, l, lp))
        if f == "alphabet" and rows * cols > 50:
            assert info[i, 12:16].all()                                         # all four modes occur
    assert ctx.pack_bound(lp) == pkg.pack_bound(display[0], display[1], lp)


def test_luma_position_0_changes_no_byte(contexts, restated):
    ctx = contexts((48, 32))
    mv, lv = content(2, 3, "alphabet", "sparse", 5)
    noisy = lv.copy()
    noisy[:, :, :16, 0] = np.random.default_rng(3).integers(-32768, 32768, size=(2, 3, 16))
    blank = np.zeros_like(lv)
    blank[:, :, :16, 0] = 2115                     # ... not even where nothing else is coded: the macroblocks are skipped
    data, info = pack(ctx, [(mv, lv), (mv, noisy), (mv, blank)])
    want = restated(("pos0", 0), mv, lv)
    same(data, info, 0, want, "as it is")
    same(data, info, 1, want, "luma position 0 set")
    assert info[2, 0] & 7 == 0 and info[2, 11] == 6


def test_carries(contexts, restated):
    """a carry into a finished byte of a first partition and of a token partition (seeds found on the CPU), and one that runs
    through 0xFF bytes (made on purpose): counted in the restatement, coded alike on the device"""
    first = content(9, 11, "far", "zero", 897)
    want = restated(("carry", "first"), *first)
    assert want["carries"][0][0] >= 1
    data, info = pack(contexts((176, 144)), [first])
    same(data, info, 0, want, "first partition")
    tokens, through = content(2, 3, "alphabet", "edges", 1937), (None, R.carry_levels())
    for what, job, lp in (("tokens", tokens, 1), ("through 0xFF", through, 0)):
        want = restated(("carry", what), *job, log2_parts=lp)
        assert sum(c[what != "tokens"] for c in want["carries"][1:]) >= 1
        data, info = pack(contexts((48, 32)), [job], log2_parts=lp)
        same(data, info, 0, want, what)


def test_many_jobs_qindex_per_job_and_other_references(contexts, restated):
    """1030 jobs cross the launch's job table and, with ten qindex values, its header table; 40 jobs at 1920x1080 cross the
    scratch bound; reference frames 2 and 3; strides larger than the sizes; one job"""
    ctx = contexts((48, 32))
    kinds = [content(2, 3, FIELDS[k % 4], LEVELS[(k // 2) % 4], 70 + k) for k in range(8)]
    qs = [3 * (i % 10) + 7 for i in range(1030)]
    jobs = [kinds[i % 8] for i in range(1030)]
    data, info = pack(ctx, jobs, cap=8192, qindex=qs, log2_parts=1, ref_frame=2, strided=True, sign_bias_golden=1)
    for i in range(1030):
        same(data, info, i, restated(("many", i % 8), *jobs[i], qindex=qs[i], log2_parts=1, ref_frame=2, sign_bias_golden=1), i)
    data, info = pack(ctx, jobs[5:6], cap=8192, ref_frame=3, prob_gf=3, version=2, show_frame=0, refresh_last=0, copy_buffer_to_gf=1)
    same(data, info, 0, restated(("one", 5), *jobs[5], ref_frame=3, prob_gf=3, version=2, show_frame=0, refresh_last=0, copy_buffer_to_gf=1), "one job")
    # eight regions of 7.2 MB a job (the bound of nine rows of 120 macroblocks; the cap is larger): 37 jobs fill the scratch
    big = contexts((1920, 1080))
    pair = [content(68, 120, "far", "zero", 90), content(68, 120, "equal", "zero", 91)]
    assert 40 * 8 * 6672 * 120 * 9 > 2 << 30 > 8 * 6672 * 120 * 9
    data, info = pack(big, [pair[i % 2] for i in range(40)], cap=8 << 20, log2_parts=3)
    for i in range(40):
        same(data, info, i, restated(("bound", i % 2), *pair[i % 2], log2_parts=3), i)


def test_statuses(contexts, restated):
    """what is refused by status: the job's frame bytes are 0, its neighbours in the call are untouched"""
    ctx = contexts((48, 32))
    mv, lv = content(2, 3, "alphabet", "sparse", 5)
    good = restated(("status", "good"), mv, lv)
    odd = mv.copy(); odd[0, 1, 1] += 1
    wide = np.zeros_like(mv); wide[0, 0, 0] = 2048                      # a difference of 1024 coded units
    edge = np.zeros_like(mv); edge[0, 0, 0] = 2046                      # 1023: legal
    big = lv.copy(); big[1, 2, 17, 5] = 2115
    legal = lv.copy(); legal[1, 2, 3, 0] = 2115                         # the same level where nothing is coded
    top = lv.copy(); top[1, 2, 17, 5] = -2114
    jobs = [(mv, lv), (odd, lv), (mv, lv), (wide, lv), (edge, lv), (mv, big), (mv, legal), (mv, top), (mv, lv)]
    data, info = pack(ctx, jobs)
    for i in (0, 2, 6, 8):
        same(data, info, i, good, i)
    for i, bit in ((1, R.BAD_VECTOR), (3, R.BAD_VECTOR), (5, R.BAD_LEVEL)):
        assert info[i, 0] & 7 == bit and info[i, 1] == 0, (i, info[i].tolist())
        assert info[i, 0] == R.restate(*jobs[i])["status"]
    same(data, info, 4, R.restate(edge, lv), "a difference of 1023")
    same(data, info, 7, R.restate(mv, top), "a level of -2114")
    # cap: the larger frame rounded up fits; 16 less and it alone overflows
    small = content(2, 3, "zero", "zero", 1)
    n = len(good["data"])
    cap = (n + 15) // 16 * 16
    data, info = pack(ctx, [small, (mv, lv), small], cap=cap)
    same(data, info, 1, good, "cap fits")
    data, info = pack(ctx, [small, (mv, lv), small], cap=cap - 16)
    assert info[1, 0] & 7 == R.OVERFLOW and info[1, 1] == 0 and info[1, 2:11].tolist() == good["info"][2:11].tolist()
    for i in (0, 2):
        same(data, info, i, R.restate(*small), "beside an overflow")
    data, info = pack(ctx, [(mv, lv)], cap=16)
    assert info[0, 0] & 7 == R.OVERFLOW and info[0, 1] == 0


def coded(ctx, fb):
    """the three coded planes of a frame buffer as downloaded"""
    return [np.ascontiguousarray(p) for p in SC.planes(ctx.download_full(fb), ctx.g)]


def test_closure_with_the_decoder(pkg):
    """pictures to bytes without the host: a key frame and a second picture at 48x32; frames_motion (d = 4), frames_subpel,
    frames_quant at qindex 40 (six-tap, levels), frames_pack with loop filter level 0; the frame, parsed and decoded by the
    product, equals frames_quant's rec byte for byte, and its bytes are the restatement's"""
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
        second = TR.noisy([((moved(p, 2 >> (i > 0), -1) + moved(p, 2 >> (i > 0), -2) + 1) >> 1).astype(np.uint8) for i, p in enumerate(key)], 5, 2)
        second[0] = np.clip(second[0].astype(np.int64) + 4 + np.arange(w) // 8, 0, 255).astype(np.uint8)
        for i, p in enumerate(second):                      # a region the reference already holds: the last macroblock is skipped
            s = 16 >> (i > 0)
            p[s:2 * s, 2 * s:3 * s] = key[i][s:2 * s, 2 * s:3 * s]
        ctx.upload_frame(5, picture_into(np.random.default_rng(1).integers(0, 256, ctx.g.frame_size, dtype=np.uint8), ctx.g, second))
        jobs = [(5, last)]
        whole, _ = ctx.frames_motion(jobs, 4, planes=())
        mv, _ = ctx.frames_subpel(jobs, start=whole, planes=())
        got = ctx.frames_quant(jobs, mv, q, filter="sixtap", stage="levels", want=("coef", "rec"))
        data, info = ctx.frames_pack(mv, got["coef"], qindex=q, filter_level=0, cap=4096)
        frames = P.pack_frames(data, info)
        info = info.cpu().numpy()
        vec = mv[0].cpu().numpy()
        assert info[0, 0] == 0 and info[0, 11] >= 1 and (vec & 7).any() and len(frames[0]) == info[0, 1]
        want = R.restate(vec, got["coef"][0].cpu().numpy(), qindex=q, filter_level=0)
        assert frames[0] == want["data"] and info[0].tolist() == want["info"].tolist()
        hdr2 = ctx.parse_into_slot(parser, frames[0], 0)
        ctx.upload(0)
        r = parser.refs
        assert r.lst_idx == last and r.new_idx != 5
        ctx.decode([(0, r.new_idx, (r.lst_idx, r.gld_idx, r.alt_idx))], P.STAGE_ALL)
        ctx.sync()
        decoded = TR.pack(coded(ctx, r.new_idx), w, h)
        rec = got["rec"][0].cpu().numpy()
        assert np.array_equal(decoded, rec), np.flatnonzero(decoded != rec)[:8].tolist()
        assert not np.array_equal(rec, TR.pack(second, w, h)) and hdr2.base_qindex == q
    finally:
        parser.close()
        ctx.close()


def raw_call(ctx, P, n, mv, mv_stride, coef, coef_stride, dst, dst_stride, cap, info, qindex=40, jq=None, **fields):
    """vp8hip_frames_pack_async itself, on pointers: -> its status"""
    p = P.PackParams()
    for name, v in {**P.PACK_DEFAULTS, **fields}.items():
        setattr(p, name, v)
    p.qindex = qindex
    keep = None if jq is None else (ctypes.c_uint8 * len(jq))(*jq)
    if keep is not None:
        p.job_qindex = keep
    vp = ctypes.c_void_p
    return ctx.L.vp8hip_frames_pack_async(ctx.h, n, ctypes.byref(p), vp(mv) if mv else None, mv_stride, vp(coef) if coef else None, coef_stride,
                                          vp(dst) if dst else None, dst_stride, cap, vp(info) if info else None)


def test_the_wrapper_and_the_refusals(pkg, contexts):
    """shapes and types, out_* filled and returned, pack_frames, what the wrapper and the call refuse"""
    P = pkg
    ctx = contexts((48, 32))
    mv_a, lv_a = content(2, 3, "alphabet", "sparse", 5)
    n = 3
    odd = mv_a.copy(); odd[1, 0, 0] = 3
    mv = torch.from_numpy(np.stack([mv_a, odd, mv_a])).to("cuda:0")
    coef = torch.from_numpy(np.stack([lv_a] * n)).to("cuda:0")
    bound = ctx.pack_bound(2)
    assert bound == P.pack_bound(48, 32, 2) and bound % 16 == 0
    data, info = ctx.frames_pack(mv, coef, log2_parts=2)
    assert data.dtype == torch.uint8 and tuple(data.shape) == (n, bound) and info.dtype == torch.int32 and tuple(info.shape) == (n, 16)
    frames = P.pack_frames(data, info)
    want = R.restate(mv_a, lv_a, log2_parts=2)["data"]
    assert frames[0] == frames[2] == want and frames[1] is None
    out_data = torch.zeros((n, 1024), dtype=torch.uint8, device="cuda:0")
    out_info = torch.zeros((n, 16), dtype=torch.int32, device="cuda:0")
    d2, i2 = ctx.frames_pack(mv, coef, log2_parts=2, out_data=out_data, out_info=out_info)
    assert d2 is out_data and i2 is out_info and torch.equal(i2, info) and P.pack_frames(d2, i2) == frames
    zero = P.pack_frames(*ctx.frames_pack(None, coef))[0]
    assert zero == R.restate(None, lv_a)["data"]
    for bad in (dict(qindex=128), dict(qindex=[40, 40]), dict(qindex=[40, 40, 200]), dict(deltas=(0, 0, 0, 0, 16)), dict(ref_frame=0), dict(log2_parts=4),
                dict(prob_intra=0), dict(prob_gf=256), dict(cap=100), dict(cap=0), dict(nonsense=1), dict(filter_level=64), dict(version=4),
                dict(out_data=torch.zeros((n, 1024), dtype=torch.int8, device="cuda:0")), dict(out_info=torch.zeros((n, 8), dtype=torch.int32, device="cuda:0")),
                dict(out_data=torch.zeros((n + 1, 1024), dtype=torch.uint8, device="cuda:0")), dict(out_data=torch.zeros((n, 1024), dtype=torch.uint8))):
        with pytest.raises((ValueError, RuntimeError)):
            ctx.frames_pack(mv, coef, **bad)
    for bad_mv, bad_coef in ((mv[:2], coef), (mv.to(torch.int32), coef), (mv, coef.to(torch.int32)), (mv, coef[:, :1]), (mv.cpu(), coef), (mv, coef.cpu())):
        with pytest.raises(ValueError):
            ctx.frames_pack(bad_mv, bad_coef)
    # the call itself, on pointers
    cap, msize, csize = 1024, 4 * 6, 800 * 6
    dst = torch.full((8 * cap,), 0xA5, dtype=torch.uint8, device="cuda:0")
    inf = torch.full((8 * 16,), -1, dtype=torch.int32, device="cuda:0")
    ok = dict(n=n, mv=mv.data_ptr(), mv_stride=msize, coef=coef.data_ptr(), coef_stride=csize, dst=dst.data_ptr(), dst_stride=cap, cap=cap, info=inf.data_ptr())

    def call(**kw):
        return raw_call(ctx, P, **{**ok, **kw})
    assert call() == 0
    ctx.sync()
    filled = (dst.clone(), inf.clone())
    assert_destinations_refused(ctx, lambda k, d, s: call(n=k, dst=d, dst_stride=s), dst.data_ptr(), cap, 16)
    assert_destinations_refused(ctx, lambda k, d, s: call(n=k, coef=d, coef_stride=s), coef.data_ptr(), csize, 16)
    assert_destinations_refused(ctx, lambda k, d, s: call(n=k, mv=d, mv_stride=s), mv.data_ptr(), msize, 2, null=False)
    assert call(info=None) == -2 and call(info=inf.data_ptr() + 2) == -2 and call(info=np.zeros(64, np.int32).ctypes.data) == -2
    assert call(n=0) == -2 and call(n=-1) == -2
    assert call(cap=cap + 16) == -2 and call(cap=cap - 8) == -2 and call(cap=0) == -2 and call(cap=8) == -2
    assert call(dst=coef.data_ptr(), dst_stride=csize) == -2 and call(info=dst.data_ptr()) == -2 and call(dst=mv.data_ptr(), cap=16, dst_stride=16) == -2
    assert call(info=coef.data_ptr()) == -2 and call(info=mv.data_ptr()) == -2
    for bad in (dict(qindex=-1), dict(qindex=128), dict(jq=[1, 2, 128]), dict(version=4), dict(show_frame=2), dict(filter_type=-1), dict(filter_level=64),
                dict(sharpness=8), dict(ref_frame=0), dict(ref_frame=4), dict(refresh_last=2), dict(refresh_golden=2), dict(refresh_alt=-1),
                dict(copy_buffer_to_gf=3), dict(copy_buffer_to_arf=3), dict(sign_bias_golden=2), dict(sign_bias_alt=2), dict(log2_parts=4),
                dict(log2_parts=-1), dict(prob_skip_false=0), dict(prob_intra=256), dict(prob_last=0), dict(prob_gf=0)):
        assert call(**bad) == -2, bad
    ctx.sync()
    assert torch.equal(dst, filled[0]) and torch.equal(inf, filled[1])         # nothing was enqueued by any of them
    assert b"vp8hip_frames_pack_async" in ctx.L.vp8hip_last_error(ctx.h)


def test_pack_refusal_texts(pkg):
    """What vp8hip_last_error says after each refusal of the three packer calls (vp8hip_frames_pack_async, _pack_adapt_async,
    _pack_key_async), and, by two faults at once, which check comes first: the texts the library gave before the three calls shared
    their host path.  48x32 -- 3 x 2 macroblocks, the smallest size at which every check is reachable --, one job (two where the
    second job's qindex is the fault) and 16 KB of device memory; every call here is refused and nothing is enqueued.  A
    destination too small is one that begins 16 bytes too near the end of its allocation.  (The alignment refusal prints a pointer
    and is left out.)"""
    P = pkg
    ctx = P.Vp8Hip(0)
    try:
        ctx.configure(48, 32, 2, 1)
        L, vp = ctx.L, ctypes.c_void_p
        mem = torch.empty((16384,), dtype=torch.uint8, device="cuda:0")
        d = mem.data_ptr()
        base, asize = hip_range(d)
        end = base + asize
        assert d % 16 == 0 and end % 16 == 0 and ctx.pack_bound(0) == 40288
        # a job's bytes: dst 64 (the cap), info 64 (128: the adapt call's), counts 4864, probs 1104, mv 24, coef 4800, modes 192
        at = dict(dst=d, info=d + 256, counts=d + 512, probs_out=d + 5632, mv=d + 6784, coef=d + 6912, probs_in=d + 11776, modes=d + 12928)

        def params(cls, defaults, qindex, job_qindex, fields):
            p = cls()
            for name, v in {**defaults, **{k: v for k, v in fields.items() if k != "delta"}}.items():
                setattr(p, name, v)
            p.delta = (ctypes.c_int * 5)(*fields.get("delta", (0, 0, 0, 0, 0)))
            p.qindex = qindex
            jq = (ctypes.c_uint8 * len(job_qindex))(*job_qindex) if job_qindex else None
            if jq:
                p.job_qindex = jq
            return p, jq

        def pack(n=1, qindex=40, job_qindex=None, cap=64, stride=64, mvs=24, cs=4800, null=(), **kw):
            a = {k: None if k in null else kw.pop(k, v) for k, v in at.items()}
            p, jq = params(P.PackParams, P.PACK_DEFAULTS, qindex, job_qindex, kw)
            return L.vp8hip_frames_pack_async(ctx.h, n, None if "p" in null else ctypes.byref(p), a["mv"], mvs, a["coef"], cs, a["dst"], stride, cap, a["info"])

        def adapt(n=1, qindex=40, job_qindex=None, cap=64, stride=64, mvs=24, cs=4800, flags=15, rep=1, ps=1104, null=(), **kw):
            a = {k: None if k in null else kw.pop(k, v) for k, v in at.items()}
            p, jq = params(P.PackParams, P.PACK_DEFAULTS, qindex, job_qindex, kw)
            ad = P.PackAdapt(flags, rep, a["probs_in"], ps)
            return L.vp8hip_frames_pack_adapt_async(ctx.h, n, None if "p" in null else ctypes.byref(p), None if "a" in null else ctypes.byref(ad), a["mv"],
                                                    mvs, a["coef"], cs, a["dst"], stride, cap, a["info"], a["counts"], a["probs_out"])

        def key(n=1, qindex=40, job_qindex=None, cap=64, stride=64, mos=192, cs=4800, null=(), **kw):
            a = {k: None if k in null else kw.pop(k, v) for k, v in at.items()}
            p, jq = params(P.PackKeyParams, P.PACK_KEY_DEFAULTS, qindex, job_qindex, kw)
            return L.vp8hip_frames_pack_key_async(ctx.h, n, None if "p" in null else ctypes.byref(p), a["modes"], mos, a["coef"], cs, a["dst"], stride, cap,
                                                  a["info"])

        def inter(version=0, flags="1 0 1 0 0 0 0", level=0, sharp=0, deltas="0 0 0 0 0", ref=1, copies="0 0", parts=0, probs="200 150 140 100"):
            return (f": version {version} (0..3), flags {flags} (0, 1), filter level {level} (0..63), sharpness {sharp} (0..7), deltas {deltas} (-15..15), "
                    f"ref_frame {ref} (1..3), buffer copies {copies} (0..2), log2_parts {parts} (0..3), probabilities {probs} (1..255)")

        def intra(version=0, flags="1 0 0 0", level=0, sharp=0, deltas="0 0 0 0 0", parts=0, skip=200):
            return (f": version {version} (0..3), flags {flags} (0, 1), filter level {level} (0..63), sharpness {sharp} (0..7), deltas {deltas} (-15..15), "
                    f"log2_parts {parts} (0..3), prob_skip_false {skip} (1..255)")
        assert inter() == (": version 0 (0..3), flags 1 0 1 0 0 0 0 (0, 1), filter level 0 (0..63), sharpness 0 (0..7), deltas 0 0 0 0 0 (-15..15), ref_frame 1 "
                           "(1..3), buffer copies 0 0 (0..2), log2_parts 0 (0..3), probabilities 200 150 140 100 (1..255)")
        assert intra() == (": version 0 (0..3), flags 1 0 0 0 (0, 1), filter level 0 (0..63), sharpness 0 (0..7), deltas 0 0 0 0 0 (-15..15), log2_parts 0 (0..3), "
                           "prob_skip_false 200 (1..255)")
        fit = " frames of {} bytes, {} apart, do not fit in the destination's allocation"
        inter_only = [
            (dict(null=("p",)), ": bad arguments"),
            (dict(version=-1), inter(version=-1)), (dict(show_frame=2), inter(flags="2 0 1 0 0 0 0")), (dict(filter_type=-1), inter(flags="1 -1 1 0 0 0 0")),
            (dict(refresh_last=2), inter(flags="1 0 2 0 0 0 0")), (dict(refresh_golden=2), inter(flags="1 0 1 2 0 0 0")),
            (dict(refresh_alt=-1), inter(flags="1 0 1 0 -1 0 0")), (dict(sign_bias_golden=2), inter(flags="1 0 1 0 0 2 0")),
            (dict(sign_bias_alt=2), inter(flags="1 0 1 0 0 0 2")), (dict(filter_level=64), inter(level=64)), (dict(sharpness=8), inter(sharp=8)),
            (dict(delta=(0, 0, 16, 0, 0)), inter(deltas="0 0 16 0 0")), (dict(delta=(0, 0, 0, 0, -16)), inter(deltas="0 0 0 0 -16")),
            (dict(ref_frame=0), inter(ref=0)), (dict(ref_frame=4), inter(ref=4)), (dict(copy_buffer_to_gf=3), inter(copies="3 0")),
            (dict(copy_buffer_to_arf=-1), inter(copies="0 -1")), (dict(log2_parts=4), inter(parts=4)), (dict(prob_skip_false=0), inter(probs="0 150 140 100")),
            (dict(prob_intra=256), inter(probs="200 256 140 100")), (dict(prob_last=0), inter(probs="200 150 0 100")),
            (dict(prob_gf=256), inter(probs="200 150 140 256")),
            (dict(mvs=20), " (mv): stride 20 below the frame's 24 bytes"),
            (dict(mv=at["dst"]), ": dst and mv overlap"), (dict(mv=at["info"]), ": info and mv overlap"),
            # two faults: the parameters before the quantiser; of two inputs the vectors first; an input's stride before an overlap
            (dict(version=4, qindex=128), inter(version=4)),
            (dict(mvs=20, cs=4784), " (mv): stride 20 below the frame's 24 bytes"),
            (dict(mvs=20, info=at["dst"]), " (mv): stride 20 below the frame's 24 bytes"),
            (dict(coef=at["dst"], mv=at["info"]), ": dst and coef overlap")]
        pack_only = [(dict(info=end - 64 + 16), " (info): 1" + fit.format(64, 64))]
        adapt_only = [
            (dict(null=("a",)), ": bad arguments"),
            (dict(flags=16), ": flags 16 (VP8HIP_ADAPT_* bits), refresh_entropy_probs 1 (0, 1)"),
            (dict(flags=-1), ": flags -1 (VP8HIP_ADAPT_* bits), refresh_entropy_probs 1 (0, 1)"),
            (dict(rep=2), ": flags 15 (VP8HIP_ADAPT_* bits), refresh_entropy_probs 2 (0, 1)"),
            (dict(info=end - 128 + 16), " (info): 1" + fit.format(128, 128)),
            (dict(counts=end - 4864 + 16), " (counts): 1" + fit.format(4864, 4864)),
            (dict(probs_out=end - 1104 + 16), " (probs_out): 1" + fit.format(1104, 1104)),
            (dict(ps=1088), " (probs_in): stride 1088 below the frame's 1104 bytes"),
            (dict(counts=at["dst"]), ": dst and counts overlap"), (dict(probs_out=at["dst"]), ": dst and probs_out overlap"),
            (dict(probs_in=at["dst"]), ": dst and probs_in overlap"), (dict(counts=at["info"]), ": info and counts overlap"),
            (dict(probs_out=at["info"]), ": info and probs_out overlap"), (dict(probs_in=at["info"]), ": info and probs_in overlap"),
            (dict(probs_out=at["counts"]), ": counts and probs_out overlap"), (dict(mv=at["counts"]), ": counts and mv overlap"),
            (dict(coef=at["counts"]), ": counts and coef overlap"), (dict(probs_in=at["counts"]), ": counts and probs_in overlap"),
            (dict(mv=at["probs_out"]), ": probs_out and mv overlap"), (dict(coef=at["probs_out"]), ": probs_out and coef overlap"),
            (dict(probs_in=at["probs_out"]), ": probs_out and probs_in overlap"),
            # two faults: cap before the adapt call's own parameters, those before the memory; the outputs before the inputs
            (dict(cap=24, flags=16), ": cap 24 (a multiple of 16, 16 .. the stride 64)"),
            (dict(flags=16, mvs=20), ": flags 16 (VP8HIP_ADAPT_* bits), refresh_entropy_probs 1 (0, 1)"),
            (dict(probs_out=end - 1104 + 16, mvs=20), " (probs_out): 1" + fit.format(1104, 1104)),
            (dict(ps=1088, counts=at["dst"]), " (probs_in): stride 1088 below the frame's 1104 bytes")]
        key_only = [
            (dict(null=("p",)), ": bad arguments"), (dict(null=("modes",)), ": bad arguments"),
            (dict(version=4), intra(version=4)), (dict(show_frame=-1), intra(flags="-1 0 0 0")), (dict(color_space=2), intra(flags="1 2 0 0")),
            (dict(clamping_type=2), intra(flags="1 0 2 0")), (dict(filter_type=2), intra(flags="1 0 0 2")), (dict(filter_level=-1), intra(level=-1)),
            (dict(sharpness=8), intra(sharp=8)), (dict(delta=(-16, 0, 0, 0, 0)), intra(deltas="-16 0 0 0 0")), (dict(log2_parts=-1), intra(parts=-1)),
            (dict(prob_skip_false=256), intra(skip=256)),
            (dict(info=end - 64 + 16), " (info): 1" + fit.format(64, 64)),
            (dict(mos=188), " (modes): stride 188 below the frame's 192 bytes"),
            (dict(modes=at["dst"]), ": dst and modes overlap"), (dict(modes=at["info"]), ": info and modes overlap"),
            (dict(version=4, qindex=128), intra(version=4)),
            (dict(mos=188, cs=4784), " (modes): stride 188 below the frame's 192 bytes"),
            (dict(coef=at["dst"], modes=at["dst"]), ": dst and modes overlap")]
        for call, who, own in ((pack, "vp8hip_frames_pack_async", inter_only + pack_only), (adapt, "vp8hip_frames_pack_adapt_async", inter_only + adapt_only),
                               (key, "vp8hip_frames_pack_key_async", key_only)):
            shared = [
                (dict(n=0), ": bad arguments"), (dict(null=("coef",)), ": bad arguments"), (dict(null=("dst",)), ": bad arguments"),
                (dict(null=("info",)), ": bad arguments"),
                (dict(qindex=128), ": qindex 128 (0..127)"), (dict(qindex=-1), ": qindex -1 (0..127)"),
                (dict(n=2, job_qindex=(5, 200)), ": job_qindex[1] = 200 (0..127)"),
                (dict(cap=0), ": cap 0 (a multiple of 16, 16 .. the stride 64)"), (dict(cap=24), ": cap 24 (a multiple of 16, 16 .. the stride 64)"),
                (dict(cap=80), ": cap 80 (a multiple of 16, 16 .. the stride 64)"),
                (dict(dst=end - 64 + 16), " (dst): 1" + fit.format(64, 64)),
                (dict(cs=4784), " (coef): stride 4784 below the frame's 4800 bytes"),
                (dict(info=at["dst"]), ": dst and info overlap"), (dict(coef=at["dst"]), ": dst and coef overlap"),
                (dict(coef=at["info"]), ": info and coef overlap"),
                # two faults: the arguments first, then the quantiser -- job_qindex where it is given, whatever qindex is --, then cap,
                # then the memory, a span's own fault before an overlap, the overlaps in the order of the outputs
                (dict(n=0, version=4), ": bad arguments"), (dict(qindex=128, cap=0), ": qindex 128 (0..127)"),
                (dict(qindex=128, job_qindex=(200,)), ": job_qindex[0] = 200 (0..127)"),
                (dict(qindex=128, job_qindex=(5,), cap=24), ": cap 24 (a multiple of 16, 16 .. the stride 64)"),
                (dict(n=2, job_qindex=(5, 200), cap=0), ": job_qindex[1] = 200 (0..127)"),
                (dict(cap=80, cs=4784), ": cap 80 (a multiple of 16, 16 .. the stride 64)"),
                (dict(dst=end - 64 + 16, cs=4784), " (dst): 1" + fit.format(64, 64)),
                (dict(cs=4784, info=at["dst"]), " (coef): stride 4784 below the frame's 4800 bytes"),
                (dict(info=at["dst"], coef=at["info"]), ": dst and info overlap")]
            for kw, text in shared + own:
                assert call(**kw) == -2, (who, kw)
                assert L.vp8hip_last_error(ctx.h).decode() == (who + text)[:255], (who, kw)     # (the context keeps 255 characters)
    finally:
        ctx.close()
