"""CPU: the launches of different frames that tests/test_gpu_inter_batches.py decodes hold what they are there for (tests/batch_testlib.py)
-- for every (size, n, seed) that module uses, so that a change of seed or of the generator cannot quietly lose the point of a GPU
test: which classes and versions share a wave, who the last job without a partner is, that no two neighbours are the same job,
that every slot and triple occurs, that no destination is a reference."""
import numpy as np
import pytest

from batch_testlib import (ALL_CLASS_PAIRS, ALL_VERSION_PAIRS, CHAIN_CASES, FORMS_CASE, INTRA, KEY, LAUNCH_CASES, NOINTRA, NSLOTS, STAGE_CASES,
                           WRAP_SIZE, check_frames, check_plan, content, extend_borders, inter_batch, wrap_n)
from vp8_testlib import bordered_area_equal, load_package, oracle_decode, synth_ir

CU_COUNTS = (256, 304, 64, 8)                 # an MI355X, and what a partitioned or another device would report
CASES = sorted(set(LAUNCH_CASES + STAGE_CASES + CHAIN_CASES + (FORMS_CASE,) + tuple(WRAP_SIZE[:2] + (wrap_n(cu), WRAP_SIZE[2]) for cu in CU_COUNTS)))


@pytest.mark.parametrize("w,h,n,seed", CASES)
def test_the_order_covers_what_it_promises(w, h, n, seed):
    check_plan(inter_batch(w, h, n, seed))


# what jobs (2p, 2p + 1) show at each launch size, spelled out: (class pairs, pairs of different versions among inter jobs)
COVERS = {
    5: ({(NOINTRA, INTRA), (INTRA, NOINTRA)}, {(0, 1), (1, 0)}),
    7: ({(NOINTRA, INTRA), (INTRA, NOINTRA), (KEY, INTRA)}, {(0, 1), (1, 0)}),
    9: ({(NOINTRA, INTRA), (INTRA, NOINTRA), (KEY, INTRA), (INTRA, KEY)}, {(0, 1), (1, 0)}),
    21: (ALL_CLASS_PAIRS, {(0, 1), (1, 0), (2, 3), (3, 2), (0, 2)}),
    37: (ALL_CLASS_PAIRS, ALL_VERSION_PAIRS),
}


@pytest.mark.parametrize("w,h,n,seed", CASES)
def test_pairs_by_launch_size(w, h, n, seed):
    cls, ver = inter_batch(w, h, n, seed).pair_coverage()
    want_cls, want_ver = COVERS[min(n, 37)]
    assert want_cls <= cls and want_ver <= ver, (sorted(want_cls - cls), sorted(want_ver - ver))
    assert len(ALL_CLASS_PAIRS) == 9 and len(ALL_VERSION_PAIRS) == 12


def test_last_jobs_are_a_key_frame_and_an_inter_frame_without_intra():
    """the last job has no B half: among the launches of different inter frames, and among all cases, both kinds end one"""
    assert {inter_batch(*c).classes[-1] for c in LAUNCH_CASES} == {KEY, NOINTRA}
    assert {inter_batch(*c).classes[-1] for c in STAGE_CASES} == {KEY, NOINTRA}


@pytest.mark.parametrize("w,h,seed,decoded", sorted({(c[0], c[1], c[3], c == FORMS_CASE) for c in CASES}))
def test_the_twelve_frames_are_what_the_table_says(w, h, seed, decoded):
    check_frames(content(w, h, seed, decoded))


def test_a_plan_is_a_function_of_its_arguments():
    """the same arguments give the same jobs in a fresh generator; another n keeps the frames and the pool (so that launches of
    different sizes can follow each other over one set of slots), another seed changes them"""
    inter_batch.cache_clear()
    a = inter_batch(48, 32, 37, 1).jobs
    inter_batch.cache_clear()
    assert inter_batch(48, 32, 37, 1).jobs == a
    assert inter_batch(48, 32, 9, 1).content is inter_batch(48, 32, 37, 1).content
    assert inter_batch(48, 32, 37, 2).jobs != a
    assert inter_batch(48, 32, 37, 2).frames[2][1].tobytes() != inter_batch(48, 32, 37, 1).frames[2][1].tobytes()


def test_expected_buffers_are_shared_and_read_only():
    p = inter_batch(48, 32, 37, 1)
    j = next(i for i in range(p.n) if p.classes[i] == INTRA)
    o = p.expected(j)
    assert p.expected(j) is o and not o.flags.writeable
    again = np.zeros(p.g.frame_size, np.uint8)
    slot, t = p.jobs[j]
    oracle_decode(*p.frames[slot], again, tuple(p.pool[k] for k in p.triples[t]), 7)
    assert np.array_equal(again, o)
    # the triple matters to an inter frame, not to a key frame
    other = (t + 1) % len(p.triples)
    assert not np.array_equal(p.content.expected(slot, other), o)
    k = next(s for s in range(NSLOTS) if p.frames[s][0].frame_type == 0)
    assert p.content.expected(k, 0) is p.content.expected(k, 3)


@pytest.mark.parametrize("w,h,n,seed", [LAUNCH_CASES[0], LAUNCH_CASES[1]])
def test_mixed_up_wave_partners_would_show(w, h, n, seed):
    """What the comparison on the GPU can see, shown with the oracle: had half B of a wave taken half A's job, A's header (version,
    dequantiser, filter) or A's references, its frame would not be the one expected -- for every pair (2p, 2p + 1) where the mix-up
    means anything: two inter frames for the header, an inter frame that reads references for the triple."""
    p = inter_batch(w, h, n, seed)
    shown_hdr = shown_refs = 0
    for a in range(0, n - 1, 2):
        b = a + 1
        assert not np.array_equal(p.expected(a), p.expected(b)), p.describe(b)
        (sa, ta), (sb, tb) = p.jobs[a], p.jobs[b]
        hdr, mbs, coef, mvs = p.frames[sb]
        # (the frame that is all skipped copies noise, which no dequantiser touches and no loop filter finds smooth enough)
        if KEY not in (p.classes[a], p.classes[b]) and sa != sb and not (mbs[:, 3] & 1).all():
            o = np.zeros(p.g.frame_size, np.uint8)
            oracle_decode(p.frames[sa][0], mbs, coef, mvs, o, tuple(p.pool[k] for k in p.triples[tb]), 7)
            assert not np.array_equal(o, p.expected(b)), p.describe(b)
            shown_hdr += 1
        if p.classes[b] != KEY and (mbs[:, 2] != 0).any() and p.classes[a] != KEY and ta != tb:
            o = np.zeros(p.g.frame_size, np.uint8)
            oracle_decode(hdr, mbs, coef, mvs, o, tuple(p.pool[k] for k in p.triples[ta]), 7)
            assert not np.array_equal(o, p.expected(b)), p.describe(b)
            shown_refs += 1
    assert shown_hdr >= 3 and shown_refs >= 2, (shown_hdr, shown_refs)


def test_all_zeromv_frame_copies_its_reference():
    """the frame that is all ZEROMV and skipped, unfiltered (stages = recon): every macroblock is a copy of its reference's"""
    P = load_package()
    p = inter_batch(48, 32, 37, 1)
    slot = 9
    hdr, mbs, coef, mvs = p.frames[slot]
    g = p.g
    o = p.content.expected(slot, 1, 1)
    cols = g.aligned_w // 16
    for i in range(len(mbs)):
        r, c = divmod(i, cols)
        ref = p.pool[p.triples[1][mbs[i, 2] - 1]]
        for y in range(16):
            at = g.y_off + (16 * r + y) * g.y_stride + 16 * c
            assert np.array_equal(o[at:at + 16], ref[at:at + 16]), (i, y)


def test_extend_borders_is_the_decoders_extension():
    """a decoded frame's borders are what extend_borders makes of its coded area"""
    P = load_package()
    g = P.geom(48, 32)
    o = np.zeros(g.frame_size, np.uint8)
    oracle_decode(*synth_ir(48, 32, 5, dense=0.5), o, (None, None, None), 7)
    again = o.copy()
    rng = np.random.default_rng(1)
    keep = np.zeros(g.frame_size, bool)
    for off, stride, w, h in ((g.y_off, g.y_stride, 48, 32), (g.u_off, g.uv_stride, 24, 16), (g.v_off, g.uv_stride, 24, 16)):
        for y in range(h):
            keep[off + y * stride:off + y * stride + w] = True
    again[~keep] = rng.integers(0, 256, size=int((~keep).sum()))
    extend_borders(again, g)
    assert not bordered_area_equal(again, o, g)


def test_synth_ir_inter_share():
    """1.0 and 0.0 give no and only intra macroblocks; the header's draws come first and do not move (what the default gives for
    the seeds in use is pinned by the recorded streams of tests/golden/sizechange_ref.json)"""
    for seed in (3, 40, 1234):
        hdr = synth_ir(64, 48, seed, inter=True)[0]
        for share, intra in ((1.0, False), (0.0, True)):
            h2, mbs, _, _ = synth_ir(64, 48, seed, inter=True, inter_share=share)
            assert bytes(h2) == bytes(hdr) and ((mbs[:, 2] == 0) == intra).all()
