"""Launches of many DIFFERENT frames, key and inter, for the tests that compare vp8hip_decode with the oracle job by job.

inter_batch(w, h, n, seed) is a plan: twelve distinct IR frames (SLOTS), a pool of six reference frame buffers, five reference
triples over the pool (TRIPLES) and n jobs, each a (slot, triple), in a seeded order that puts what a launch of identical jobs
cannot show next to each other: jobs 2p and 2p + 1 share a wave in the wave-per-row kernels, so the order is built from the
PAIRS it has to contain (REQUIRED_PAIRS, as many as n has room for) and shuffled.  check_plan() asserts what the order promises;
tests/test_batch_plan_cpu.py runs it for every case the GPU module launches.

The frames, the pool and the oracle's frame buffer of every distinct (slot, triple, stages) are made once per (size, seed) and
shared by every plan and every test of that size; they are read-only."""
import functools

import numpy as np

from vp8_testlib import load_package, oracle_decode, random_frame, synth_ir

KEY, INTRA, NOINTRA = "key", "inter+intra", "inter"      # a job's class: key frame, inter frame with / without intra macroblocks
CLASSES = (KEY, INTRA, NOINTRA)

# the twelve frames: (class, version, filter_type, segmented, big, dense, what is special)
SLOTS = (
    (KEY, 0, 0, True, True, 0.5, ""),
    (KEY, 3, 1, False, False, 0.3, "filter_level 0"),
    (INTRA, 0, 0, True, True, 0.4, ""),
    (INTRA, 1, 1, False, False, 0.3, ""),
    (INTRA, 2, 0, True, False, 0.6, ""),
    (INTRA, 3, 1, True, False, 0.3, ""),
    (NOINTRA, 0, 1, True, False, 0.4, "no intra macroblock"),
    (INTRA, 1, 0, False, False, 0.3, "all intra"),
    (INTRA, 2, 1, True, False, 0.3, "filter_level 0"),
    (NOINTRA, 1, 0, True, False, 0.0, "all ZEROMV and skipped"),
    (NOINTRA, 2, 1, False, False, 0.5, "all SPLITMV, sixteen vectors"),
    (NOINTRA, 3, 0, True, False, 0.3, "no intra macroblock"),
)
NSLOTS, NPOOL = len(SLOTS), 6
# (last, golden, alt) over the pool: one buffer three times, three buffers, golden == alt, last == golden, last == alt
TRIPLES = ((0, 0, 0), (1, 2, 3), (4, 5, 5), (3, 3, 1), (5, 2, 5))
POOL_FB0, DST_FB0 = 0, NPOOL                  # frame buffers: the pool first, then job i's destination DST_FB0 + i

# What jobs (2p, 2p + 1) have to be, most telling first: (class of A, class of B, (version of A, version of B) or None).  All
# nine ordered pairs of classes -- the four among inter frames carry a pair of versions too -- then the other eight ordered pairs
# of different versions, between inter frames of any class.  A launch of n jobs holds the first (n - 1) // 2 of them.
REQUIRED_PAIRS = (
    (NOINTRA, INTRA, (0, 1)), (INTRA, NOINTRA, (1, 0)), (KEY, INTRA, None), (INTRA, KEY, None), (KEY, NOINTRA, None),
    (NOINTRA, KEY, None), (NOINTRA, NOINTRA, (2, 3)), (KEY, KEY, None), (INTRA, INTRA, (3, 2)),
) + tuple((None, None, v) for v in ((0, 2), (2, 0), (0, 3), (3, 0), (1, 2), (2, 1), (1, 3), (3, 1)))


def extend_borders(buf, g):
    """vp8_yv12_extend_frame_borders on a frame buffer, in place: 32 / 16 pixels around the coded area of every plane"""
    for off, stride, w, h, bd in ((g.y_off, g.y_stride, g.aligned_w, g.aligned_h, 32),
                                  (g.u_off, g.uv_stride, g.aligned_w // 2, g.aligned_h // 2, 16),
                                  (g.v_off, g.uv_stride, g.aligned_w // 2, g.aligned_h // 2, 16)):
        p = np.lib.stride_tricks.as_strided(buf[off - bd * stride - bd:], shape=(h + 2 * bd, w + 2 * bd), strides=(stride, 1))
        p[bd:bd + h, :bd] = p[bd:bd + h, bd:bd + 1]
        p[bd:bd + h, bd + w:] = p[bd:bd + h, bd + w - 1:bd + w]
        p[:bd] = p[bd]
        p[bd + h:] = p[bd + h - 1]
    return buf


def _without_y2(mbs, coef):
    """Macroblocks that had a Y2 block become ones without (as SPLITMV has none): the Y blocks' first coefficient is zero already and
    stays, their eobs count from 0 instead of 1, the Y2 block goes; a macroblock left without a coefficient is skipped."""
    y2 = ~np.isin(mbs[:, 0], (4, 9))
    eobs = mbs[:, 8:24]
    eobs[y2[:, None] & (eobs == 1)] = 0
    mbs[y2, 8 + 24] = 0
    coef[y2, 24 * 16:] = 0
    mbs[mbs[:, 8:33].sum(1) == 0, 3] |= 1


def _all_splitmv(w, h, seed, mbs, coef, mvs):
    """every macroblock SPLITMV with partition 3: sixteen vectors of its own, drawn as synth_ir draws them"""
    rng = np.random.default_rng(seed)
    cols, rows = (w + 15) // 16, (h + 15) // 16
    _without_y2(mbs, coef)
    mbs[:, 0], mbs[:, 5] = 9, 3
    for i in range(cols * rows):
        r, c = divmod(i, cols)
        far = 400 if mbs[i, 3] & 2 else 0
        lim_l, lim_r = -(c * 16 + 16) * 8 - far, ((cols - 1 - c) * 16 + 16) * 8 + far
        lim_t, lim_b = -(r * 16 + 16) * 8 - far, ((rows - 1 - r) * 16 + 16) * 8 + far
        mvs[i, :, 0] = rng.integers(lim_t // 2, lim_b // 2 + 1, size=16) * 2
        mvs[i, :, 1] = rng.integers(lim_l // 2, lim_r // 2 + 1, size=16) * 2


def _all_zeromv_skipped(mbs, coef, mvs):
    mbs[:, 0], mbs[:, 3], mbs[:, 5] = 7, 1, 0
    mbs[:, 8:33] = 0
    coef[:] = 0
    mvs[:] = 0


def job_class(hdr, mbs):
    if hdr.frame_type == 0:
        return KEY
    return INTRA if (mbs[:, 2] == 0).any() else NOINTRA


class Content:
    """What the plans of one (size, seed) share: frames, pool, and the oracle's buffers as they are asked for."""

    def __init__(self, w, h, seed, decoded_pool):
        P = load_package()
        self.w, self.h, self.seed, self.g = w, h, seed, P.geom(w, h)
        self.frames = []
        for s, (cls, version, ftype, segmented, big, dense, special) in enumerate(SLOTS):
            def draw(share):
                return synth_ir(w, h, 1000 * seed + 31 * s + w + h, inter=cls != KEY, version=version, filter_type=ftype,
                                dense=dense, big=big, segmented=segmented, inter_share=share)
            hdr, mbs, coef, mvs = draw(1.0 if cls == NOINTRA else 0.0 if special == "all intra" else 0.8)
            if cls == INTRA and not (mbs[:, 2] == 0).any():       # (a frame of one macroblock may have drawn "inter" for it)
                hdr, mbs, coef, mvs = draw(0.0)
            if special == "all SPLITMV, sixteen vectors":
                _all_splitmv(w, h, 77 * seed + s, mbs, coef, mvs)
            elif special == "all ZEROMV and skipped":
                _all_zeromv_skipped(mbs, coef, mvs)
            hdr.filter_level = 0 if special == "filter_level 0" else hdr.filter_level or 1 + (seed + 5 * s) % 63
            for a in (mbs, coef, mvs):
                a.flags.writeable = False
            self.frames.append((hdr, mbs, coef, mvs))
        # the pool: noise with its borders extended (a tiled form has no borders of its own: vp8_inter_pred_tiles_kernel replicates
        # the edge, so a raster form must hold what replication gives), or six decoded key frames with their IR
        self.pool, self.pool_ir = [], []
        for k in range(NPOOL):
            if decoded_pool:
                ir = synth_ir(w, h, 500 + 1000 * seed + 11 * k + w, inter=False, dense=0.4, version=k % 4, filter_type=k % 2)
                buf = np.zeros(self.g.frame_size, np.uint8)
                oracle_decode(*ir, buf, (None, None, None), 7)
                self.pool_ir.append(ir)
            else:
                buf = extend_borders(random_frame(self.g, 100 + 1000 * seed + k), self.g)
            buf.flags.writeable = False
            self.pool.append(buf)
        self._expected = {}

    def expected(self, slot, triple, stages=7):
        """the oracle's frame buffer of frame `slot` decoded from reference triple `triple` (computed once; read-only)"""
        key = (slot, triple if self.frames[slot][0].frame_type else 0, stages)
        if key not in self._expected:
            o = np.zeros(self.g.frame_size, np.uint8)
            oracle_decode(*self.frames[slot], o, tuple(self.pool[k] for k in TRIPLES[triple]), stages)
            o.flags.writeable = False
            self._expected[key] = o
        return self._expected[key]

    def slot_class(self, slot):
        return job_class(*self.frames[slot][:2])


@functools.lru_cache(maxsize=None)
def content(w, h, seed, decoded_pool=False):
    return Content(w, h, seed, decoded_pool)


def _candidates(cls, version):
    return [s for s, spec in enumerate(SLOTS) if (cls is None or spec[0] == cls) and (version is None or spec[1] == version)
            and (cls is not None or version is None or spec[0] != KEY)]


def _job_order(n, seed, last):
    """-> [(slot, triple)] * n: the first (n - 1) // 2 of REQUIRED_PAIRS (random pairs beyond them) in a shuffled order, then one job
    of class `last` without a partner.  A position takes a slot no job has used while there is one among those it may take, the
    most constrained positions first; triples likewise.  The two jobs of a pair are different frames, neighbours across pairs too
    where the position has a choice, and no job repeats the (slot, triple) of the job before it."""
    assert n % 2 == 1 and n >= 3
    rng = np.random.default_rng(7919 * seed + n)
    npairs = n // 2
    pairs = list(REQUIRED_PAIRS[:npairs]) + [(None, None, None)] * max(0, npairs - len(REQUIRED_PAIRS))
    pairs = [pairs[i] for i in rng.permutation(npairs)]
    cands = []
    for ca, cb, v in pairs:
        cands += [_candidates(ca, v and v[0]), _candidates(cb, v and v[1])]
    cands.append(_candidates(last, None))
    slots, used = [None] * n, set()
    for i in sorted(range(n), key=lambda i: (len(cands[i]), i)):
        partner = slots[i ^ 1] if (i ^ 1) < n else None       # two jobs of a wave are never the same frame
        other = slots[i - 1 if i & 1 == 0 else i + 1] if 0 <= (i - 1 if i & 1 == 0 else i + 1) < n else None
        may = [s for s in cands[i] if s != partner]
        may = [s for s in may if s != other] or may
        fresh = [s for s in may if s not in used]
        slots[i] = int(rng.choice(fresh or may))
        used.add(slots[i])
    jobs, used_t = [], set()
    for i in range(n):
        free = [t for t in range(len(TRIPLES)) if not jobs or (slots[i], t) != jobs[-1]]
        fresh = [t for t in free if t not in used_t]
        t = int(rng.choice(fresh or free))
        used_t.add(t)
        jobs.append((slots[i], t))
    return jobs


class Plan:
    def __init__(self, w, h, n, seed, decoded_pool=False):
        self.w, self.h, self.n, self.seed = w, h, n, seed
        self.content = content(w, h, seed, decoded_pool)
        self.g, self.frames, self.pool, self.pool_ir = self.content.g, self.content.frames, self.content.pool, self.content.pool_ir
        self.triples = TRIPLES
        self.last = (KEY, NOINTRA)[seed % 2]
        self.jobs = _job_order(n, seed, self.last)
        self.classes = [self.content.slot_class(s) for s, _ in self.jobs]
        self.versions = [self.frames[s][0].version for s, _ in self.jobs]

    def expected(self, j, stages=7):
        return self.content.expected(*self.jobs[j], stages)

    def launch_jobs(self, rot=0):
        """the launch as Vp8Hip.decode takes it: position i decodes job (i + rot) % n into frame buffer DST_FB0 + i; a key frame
        names no reference"""
        out = []
        for i in range(self.n):
            slot, t = self.jobs[(i + rot) % self.n]
            refs = tuple(POOL_FB0 + k for k in TRIPLES[t]) if self.frames[slot][0].frame_type else None
            out.append((slot, DST_FB0 + i, refs))
        return out

    def describe(self, j, rot=0):
        """who position j of a launch is, for a failure's message: the job, its class, its partner's, the version, the triple"""
        def one(i):
            slot, t = self.jobs[(i + rot) % self.n]
            return (f"slot {slot} ({self.classes[(i + rot) % self.n]}, version {self.versions[(i + rot) % self.n]}"
                    f"{', ' + SLOTS[slot][6] if SLOTS[slot][6] else ''}), triple {t} = pool {TRIPLES[t]}")
        partner = j ^ 1
        return (f"{self.w}x{self.h} job {j} of {self.n}: {one(j)}; "
                + (f"shares a wave with job {partner}: {one(partner)}" if partner < self.n else "no partner (last job)"))

    def pair_coverage(self):
        """-> (ordered class pairs, ordered pairs of different versions among inter jobs) that occur at some (2p, 2p + 1)"""
        cls, ver = set(), set()
        for a in range(0, self.n - 1, 2):
            cls.add((self.classes[a], self.classes[a + 1]))
            if KEY not in (self.classes[a], self.classes[a + 1]) and self.versions[a] != self.versions[a + 1]:
                ver.add((self.versions[a], self.versions[a + 1]))
        return cls, ver


@functools.lru_cache(maxsize=None)
def inter_batch(w, h, n, seed, decoded_pool=False):
    return Plan(w, h, n, seed, decoded_pool)


ALL_CLASS_PAIRS = {(a, b) for a in CLASSES for b in CLASSES}
ALL_VERSION_PAIRS = {(a, b) for a in range(4) for b in range(4) if a != b}


def promised_coverage(n):
    """what a launch of n jobs has room for: the class pairs and version pairs of the first (n - 1) // 2 REQUIRED_PAIRS"""
    req = REQUIRED_PAIRS[:n // 2]
    return {(a, b) for a, b, _ in req if a is not None}, {v for _, _, v in req if v is not None}


def check_frames(c):
    """the twelve frames of a Content hold what their table says"""
    hdrs = [f[0] for f in c.frames]
    for s, (cls, version, ftype, segmented, big, dense, special) in enumerate(SLOTS):
        hdr, mbs, coef, mvs = c.frames[s]
        assert c.slot_class(s) == cls, (s, c.slot_class(s), cls)
        assert (hdr.version, hdr.filter_type, hdr.segmentation_enabled) == (version, ftype, int(segmented)), s
        assert (hdr.filter_level == 0) == (special == "filter_level 0"), (s, hdr.filter_level)
        skipped = (mbs[:, 3] & 1) != 0
        assert not mbs[skipped, 8:33].any() and not coef[skipped].any(), s
        assert (mbs[~skipped, 8:33].sum(1) > 0).all(), s
        y2 = ~np.isin(mbs[:, 0], (4, 9))
        assert not mbs[~y2, 8 + 24].any() and not coef[y2][:, 0:256:16].any(), s       # no Y2 block / the Y blocks start at 1
        if big and len(mbs) >= 6:
            assert np.abs(coef).max() > 1000, s
        if special == "all intra":
            assert (mbs[:, 2] == 0).all(), s
        if special == "all ZEROMV and skipped":
            assert (mbs[:, 0] == 7).all() and skipped.all() and not mvs.any() and (mbs[:, 2] != 0).all(), s
        if special.startswith("all SPLITMV"):
            assert (mbs[:, 0] == 9).all() and (mbs[:, 5] == 3).all() and (mbs[:, 2] != 0).all(), s
            assert all(len({tuple(v) for v in mvs[i]}) > 8 for i in range(len(mbs))), s
    inter = [h for h in hdrs if h.frame_type]
    keys = [h for h in hdrs if not h.frame_type]
    assert len(keys) == 2 and sorted(h.filter_level == 0 for h in keys) == [False, True]
    assert {h.version for h in inter} == {0, 1, 2, 3}
    assert any(h.filter_level == 0 for h in inter) and any(h.filter_level for h in inter)
    for group in (keys, inter):
        assert {h.filter_type for h in group} == {0, 1} and {h.segmentation_enabled for h in group} == {0, 1}
    assert any(SLOTS[s][0] == KEY and SLOTS[s][4] for s in range(NSLOTS)) and any(SLOTS[s][0] != KEY and SLOTS[s][4] for s in range(NSLOTS))
    assert len({c.frames[s][1].tobytes() + c.frames[s][2].tobytes() + bytes(c.frames[s][0]) for s in range(NSLOTS)}) == NSLOTS
    assert len({p.tobytes() for p in c.pool}) == NPOOL
    assert {k for t in TRIPLES for k in t} == set(range(NPOOL))
    assert [len(set(t)) for t in TRIPLES] == [1, 3, 2, 2, 2] and len({(t[0] == t[1], t[1] == t[2], t[0] == t[2]) for t in TRIPLES}) == 5


def check_plan(p):
    """the order of a Plan holds what the module's text promises for its n"""
    assert p.n % 2 == 1 and len(p.jobs) == p.n
    cls, ver = p.pair_coverage()
    want_cls, want_ver = promised_coverage(p.n)
    assert want_cls <= cls, (p.n, sorted(want_cls - cls))
    assert want_ver <= ver, (p.n, sorted(want_ver - ver))
    if p.n >= 37:
        assert cls == ALL_CLASS_PAIRS and ver == ALL_VERSION_PAIRS
    assert p.classes[-1] == p.last and p.last in (KEY, NOINTRA)
    assert all(p.jobs[i] != p.jobs[i + 1] for i in range(p.n - 1))
    assert all(p.jobs[a][0] != p.jobs[a + 1][0] for a in range(0, p.n - 1, 2))      # (a key frame is the same whatever its triple)
    assert {t for _, t in p.jobs} == set(range(len(TRIPLES))) or p.n < len(TRIPLES)
    assert {s for s, _ in p.jobs} == set(range(NSLOTS)) or p.n < 21, sorted(set(range(NSLOTS)) - {s for s, _ in p.jobs})
    for rot in (0, 1, 2):
        launch = p.launch_jobs(rot)
        dsts = [d for _, d, _ in launch]
        refs = {f for _, _, r in launch if r for f in r}
        assert len(set(dsts)) == p.n and not refs & set(dsts)
        assert all((r is None) == (p.frames[s][0].frame_type == 0) for s, _, r in launch)
    # non-periodic: no shift of the order by 1 .. 8 jobs maps it onto itself
    if p.n >= 21:
        assert all(any(p.jobs[i] != p.jobs[i + k] for i in range(p.n - k)) for k in range(1, 9))


# every (w, h, n, seed) the GPU module launches but the one whose n follows from the device's CU count (wrap_n)
LAUNCH_CASES = ((48, 32, 37, 1), (176, 144, 21, 2), (16, 16, 9, 3), (33, 600, 7, 4), (1000, 40, 5, 5))
STAGE_CASES = ((48, 32, 37, 1), (176, 144, 21, 2))
WRAP_SIZE = (48, 32, 6)                       # w, h, seed
FORMS_CASE = (176, 144, 21, 7)                # the pool decoded, half of it on the device as tiles only
CHAIN_CASES = ((48, 32, 9, 1), (48, 32, 37, 1))


def wrap_n(num_cu):
    """jobs that wrap every persistent grid at 48x32: above the 32 * num_cu waves of the prediction kernels (a job a wave) -- so above
    the 64 * num_cu waves of vp8_inter_mb_kernel at three units a job and above num_cu pairs --, 37 more, odd"""
    return (32 * num_cu + 37) | 1
