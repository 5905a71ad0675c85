"""GPU (-m gpu): launches of many DIFFERENT frames, key and inter, against the oracle job by job, bit for bit.

vp8hip_decode decodes the same position of many streams in one launch, and much of its code means nothing for one frame or for
copies of one: frames A and B of a pair in the halves of a wave with their own header, version, dequantiser and intra flag
(vp8_recon.hip), a unit number turned into (job, chunk of 64 macroblocks) and the chunk sorted into filtered, copied and SPLITMV
lists by ballot (vp8_inter_pred.hip, vp8_inter_mb_kernel), key frames among inter frames strand after strand
(vp8_interframe_kernel), the references of all jobs collected and converted between their two forms once per launch
(vp8hip_launch.hip).  tests/batch_testlib.py makes the launches: twelve frames of every kind, five reference triples over a pool
of six buffers, and an order in which every class of frame and every version is the wave partner of every other
(tests/test_batch_plan_cpu.py holds that order to its promise).  A mismatch names the job, its class, its partner's, the version
and the triple."""
import numpy as np
import pytest

from batch_testlib import (CHAIN_CASES, DST_FB0, FORMS_CASE, LAUNCH_CASES, NPOOL, NSLOTS, POOL_FB0, STAGE_CASES, WRAP_SIZE, check_plan,
                           inter_batch, wrap_n)
from vp8_testlib import bordered_area_equal, coded_area_equal, md5_list

pytestmark = pytest.mark.gpu

WAVE_FAMILIES = ["wave", "wave1cu", "wave_split", "wave1cu_split"]
FAMILIES = WAVE_FAMILIES + ["lane", "lane_tiles2"]


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Vp8Hip(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def num_cu():
    """the device's multiprocessor count, which is what the library sizes its persistent grids by (vp8hip_create)"""
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _family(monkeypatch, family, pred_tiles=None):
    """the library's knobs as tests/test_gpu_parity.py sets them (read when a context is configured); "lane_tiles2": the lane family
    predicting from tiles whatever form the references have (VP8HIP_PRED_TILES=2)"""
    monkeypatch.setenv("VP8HIP_RECON", "simt" if family.startswith("lane") else "wave")
    if family.startswith("wave1cu"):
        monkeypatch.setenv("VP8HIP_XCU", "0")
    else:
        monkeypatch.delenv("VP8HIP_XCU", raising=False)
    if family.endswith("_split"):
        monkeypatch.setenv("VP8HIP_INTER_SPLIT", "100000")
    elif family == "wave1cu":
        monkeypatch.setenv("VP8HIP_INTER_SPLIT", "0")
    else:
        monkeypatch.delenv("VP8HIP_INTER_SPLIT", raising=False)
    if pred_tiles is None and family == "lane_tiles2":
        pred_tiles = 2
    if pred_tiles is None:
        monkeypatch.delenv("VP8HIP_PRED_TILES", raising=False)
    else:
        monkeypatch.setenv("VP8HIP_PRED_TILES", str(pred_tiles))
    for k in ("VP8HIP_SIMT_LGG", "VP8HIP_SIMT_WAVES", "VP8HIP_EAGER_RASTER"):
        monkeypatch.delenv(k, raising=False)


def _setup(ctx, plan, n=None, extra_slots=0, upload_pool=range(NPOOL)):
    """a context for the plan's size with its frames in slots 0 .. 11 and its pool in frame buffers 0 .. 5"""
    ctx.configure(plan.w, plan.h, DST_FB0 + (n or plan.n), NSLOTS + extra_slots)
    for k in upload_pool:
        ctx.upload_frame(POOL_FB0 + k, plan.pool[k])
    for s, ir in enumerate(plan.frames):
        ctx.fill_slot(s, *ir)


def _check_all(ctx, plan, family, stages=7, rot=0, what=""):
    equal = bordered_area_equal if stages == 7 else coded_area_equal
    for j in range(plan.n):
        d = equal(ctx.download_full(DST_FB0 + j), plan.expected((j + rot) % plan.n, stages), plan.g)
        assert not d, f"{family} {what}stages {stages}: {plan.describe(j, rot)}: {d}"


@pytest.mark.parametrize("w,h,n,seed", LAUNCH_CASES)
@pytest.mark.parametrize("family", FAMILIES)
def test_different_inter_frames_in_one_launch(pkg, ctx, monkeypatch, family, w, h, n, seed):
    """Every job of one launch against the oracle, whole buffers with borders.  48x32 x 37: six macroblocks, a chunk of the prediction
    kernels is mostly idle lanes, all nine class pairs; 176x144 x 21: two chunks a job, the second partial, unit -> job is a
    division; 16x16 x 9: one macroblock, too narrow for the tile reader; 33x600 x 7: 38 rows of 3 columns, row period above the
    columns in the lane family, more rows than waves in the other; 1000x40 x 5: 3 rows of 63 columns, a workgroup's waves span
    pairs."""
    _family(monkeypatch, family)
    plan = inter_batch(w, h, n, seed)
    _setup(ctx, plan)
    ctx.decode(plan.launch_jobs(), 7)
    st = ctx.stats()
    assert st.fused == int(family.startswith("lane")), (family, st.fused)
    if family == "lane_tiles2":
        assert st.pred_tiles == (1 if plan.g.aligned_w >= 32 else 0), (w, h, st.pred_tiles)
    else:
        assert st.pred_tiles == 0, (family, st.pred_tiles)          # (uploaded references have a raster form)
    _check_all(ctx, plan, family)


@pytest.mark.parametrize("w,h,n,seed", STAGE_CASES)
@pytest.mark.parametrize("family", WAVE_FAMILIES)
def test_single_stages_of_different_frames(pkg, ctx, monkeypatch, family, w, h, n, seed):
    """Reconstruction alone, reconstruction + loop filter (coded area), then everything (whole buffers), one launch after the other
    into the same buffers: the stages of every job are the oracle's."""
    _family(monkeypatch, family)
    plan = inter_batch(w, h, n, seed)
    _setup(ctx, plan)
    for stages in (1, 3, 7):
        ctx.decode(plan.launch_jobs(), stages)
        assert ctx.stats().fused == 0
        _check_all(ctx, plan, family, stages)


def _wrap_sample(n, num_cu):
    """64 jobs of a launch of n: the first and last two, the jobs either side of where a persistent grid of the three families
    starts over -- 32 * num_cu waves of the prediction kernels, 64 * num_cu waves of vp8_inter_mb_kernel at three units a job,
    num_cu pairs of the row-ordered kernels, 4 * num_cu waves of 2 .. 32 strands in the lane-per-row kernel -- and seeded others"""
    at = {0, 1, n - 2, n - 1}
    for b in [32 * num_cu, 64 * num_cu // 3, 2 * num_cu, 4 * num_cu] + [4 * num_cu * (2 << k) for k in range(5)]:
        at |= {j for j in (b - 1, b, b + 1) if 0 <= j < n}
    rng = np.random.default_rng(n)
    while len(at) < 64:
        at.add(int(rng.integers(0, n)))
    return sorted(at)


@pytest.mark.parametrize("family", ["lane", "wave_split", "wave"])
def test_a_launch_that_wraps_every_persistent_grid(pkg, ctx, num_cu, monkeypatch, family):
    """More jobs at 48x32 than any grid has waves or pairs (batch_testlib.wrap_n of the device's CU count): every block of the
    prediction kernels, of vp8_inter_mb_kernel and of the row-ordered kernels goes round its loop again, with other jobs.  Every
    job's digest from the device against the oracle's frame, and 64 buffers whole."""
    _family(monkeypatch, family)
    w, h, seed = WRAP_SIZE
    n = wrap_n(num_cu)
    assert n % 2 == 1 and n > 32 * num_cu + 36 and 3 * n > 64 * num_cu and n // 2 > num_cu
    plan = inter_batch(w, h, n, seed)
    check_plan(plan)
    _setup(ctx, plan)
    ctx.decode(plan.launch_jobs(), 7)
    assert ctx.stats().fused == int(family == "lane")
    got = md5_list(ctx, [DST_FB0 + j for j in range(n)])
    want = {}
    for j in range(n):
        if plan.jobs[j] not in want:
            want[plan.jobs[j]] = pkg.frame_md5(plan.expected(j), plan.g, w, h)
    bad = [j for j in range(n) if got[j] != want[plan.jobs[j]]]
    assert not bad, f"{family}: {len(bad)} of {n} digests differ; the first: {plan.describe(bad[0])}"
    for j in _wrap_sample(n, num_cu):
        d = bordered_area_equal(ctx.download_full(DST_FB0 + j), plan.expected(j), plan.g)
        assert not d, f"{family}: {plan.describe(j)}: {d}"


@pytest.mark.parametrize("pred_tiles", [0, 1, 2])
def test_references_in_both_forms_in_one_launch(pkg, ctx, monkeypatch, pred_tiles):
    """Pool buffers 0 .. 2 decoded by a lane launch of key frames -- tiles, no raster form --, 3 .. 5 uploaded -- raster, no tiles --,
    and triples that mix them within a job and across jobs: the launch converts what lacks the form it reads (to raster with
    VP8HIP_PRED_TILES=0, to tiles otherwise), every job equals the oracle, and the six references are afterwards what they were."""
    _family(monkeypatch, "lane", pred_tiles)
    plan = inter_batch(*FORMS_CASE, decoded_pool=True)
    _setup(ctx, plan, extra_slots=3, upload_pool=(3, 4, 5))
    for k in range(3):
        ctx.fill_slot(NSLOTS + k, *plan.pool_ir[k])
    ctx.decode([(NSLOTS + k, POOL_FB0 + k, None) for k in range(3)], 7)
    assert ctx.stats().fused == 1
    ctx.decode(plan.launch_jobs(), 7)
    st = ctx.stats()
    assert st.fused == 1 and st.pred_tiles == (0, 1, 1)[pred_tiles], (pred_tiles, st.fused, st.pred_tiles)
    _check_all(ctx, plan, "lane", what=f"VP8HIP_PRED_TILES={pred_tiles} ")
    for k in range(NPOOL):
        got = ctx.download_full(POOL_FB0 + k)
        if k < 3:
            d = bordered_area_equal(got, plan.pool[k], plan.g)
            assert not d, (pred_tiles, "reference decoded on the device", k, d)
        else:
            assert np.array_equal(got, plan.pool[k]), (pred_tiles, "uploaded reference", k)


@pytest.mark.parametrize("family", ["wave_split", "lane"])
def test_launches_of_different_sizes_back_to_back(pkg, ctx, monkeypatch, family):
    """Nine jobs, then at once 37 -- the job tables and the intra flags grow while the first launch may still read them --, then
    the 37 twice more rotated by one into the same destinations, so that every pair and strand gets other partners: after one
    sync every buffer holds the last launch's frame."""
    _family(monkeypatch, family)
    small, plan = (inter_batch(*c) for c in CHAIN_CASES)
    assert small.content is plan.content
    _setup(ctx, plan)
    ctx.decode(small.launch_jobs(), 7)
    for rot in (0, 1, 2):
        ctx.decode(plan.launch_jobs(rot), 7)
    ctx.sync()
    _check_all(ctx, plan, family, rot=2, what="after four launches ")
