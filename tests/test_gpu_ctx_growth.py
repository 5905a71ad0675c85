"""GPU (-m gpu): ONE context whose buffers grow again and again, with work in flight and across reconfigurations -- the job
tables, the digest buffer, the index list, the packed staging, the entropy decoder's input and scratch (csrc/hip/vp8hip_res.hip.h:
Buf::grow, behind the wait each call site makes).  Whatever a grown buffer carries is checked against the reference decoder's
MD5 listings: a capacity in the wrong unit, a lost wait or a buffer a reconfiguration should have kept shows as a wrong digest.
torch is imported here, before the package loads libvp8hip.so: one HIP runtime per process (frames_rgb hands out tensors)."""
import hashlib

import torch  # noqa: F401  (first: the library then shares torch's HIP runtime)
import numpy as np
import pytest

from vp8_testlib import golden_md5, ivf_path, md5_list

pytestmark = pytest.mark.gpu

NFB = 130


def _configure_and_fill(P, ctx, name):
    """the context configured for the fixture, NFB frame buffers and a slot per frame, every frame in its slot; -> frames"""
    w, h, frames = P.read_ivf(ivf_path(name))
    ctx.configure(w, h, NFB, len(frames))
    parser = P.Parser()
    try:
        for i, data in enumerate(frames):
            hdr, _ = ctx.parse_into_slot_compact(parser, data, i)
            parser.swap(hdr)
    finally:
        parser.close()
    return len(frames)


def _decode(ctx, nf, k):
    ctx.decode([(i % nf, i, None) for i in range(k)])


def _grow_through(P, ctx, name):
    """steps 1-4 of the module's docstring on a freshly configured context; nothing waits between the calls but the calls"""
    nf = _configure_and_fill(P, ctx, name)
    gold = golden_md5(name)
    want = [gold[i % nf] for i in range(NFB)]
    # the job tables, and behind each launch the digest buffer: 64 -> 70 -> 130
    for k in (2, 70, NFB):
        _decode(ctx, nf, k)
        assert ctx.frames_md5(0, k) == want[:k], (name, "frames_md5", k)
    # the packed staging: 2 frames, then 70 (in two pieces)
    for k in (2, 70):
        got = [hashlib.md5(f.tobytes()).hexdigest() for f in ctx.frames_i420(0, k)]
        assert got == want[:k], (name, "frames_i420", k)
    # the index list: 3 buffers, then 100 in any order, one of them twice
    assert md5_list(ctx, [5, 0, 129]) == [want[5], want[0], want[129]], (name, "list of 3")
    fbs = [int(v) for v in np.random.default_rng(7).permutation(NFB)[:99]]
    fbs.insert(40, fbs[3])
    assert md5_list(ctx, fbs) == [want[f] for f in fbs], (name, "list of 100")


@pytest.mark.parametrize("recon", [None, "simt"])
def test_buffers_grow_under_one_context(pkg, monkeypatch, recon):
    """recon None: the launches leave raster frames; simt: tiles, which the digests and the packing read as they are (640 is whole
    MD5 blocks wide).  176 is not: there the raster form and the any-width hash are used whatever the launch left."""
    if recon:
        monkeypatch.setenv("VP8HIP_RECON", recon)
    else:
        monkeypatch.delenv("VP8HIP_RECON", raising=False)
    P = pkg
    ctx = P.Vp8Hip(0)
    try:
        _grow_through(P, ctx, "kf_640x360")
        _grow_through(P, ctx, "kf_q0_176x144")
        nf = _configure_and_fill(P, ctx, "kf_640x360")
        _decode(ctx, nf, NFB)
        gold = golden_md5("kf_640x360")
        assert ctx.frames_md5(0, NFB) == [gold[i % nf] for i in range(NFB)]
        # the RGB scratch (a chunk of scaled frames): allocated, grown, and what went through it is the same picture twice
        small = ctx.frames_rgb([0, nf], 160, 90)
        assert 0 < ctx.rgb_scratch_bytes() < 4 * 160 * 90
        big = ctx.frames_rgb([3, nf + 3, 129], 320, 180)
        assert ctx.rgb_scratch_bytes() >= 3 * (320 * 180 * 3 // 2)
        assert torch.equal(small[0], small[1]) and torch.equal(big[0], big[1]) and not torch.equal(big[0], big[2])
        assert ctx.memory_usage()["packed_staging"] > 0
        ctx.release_staging()
        assert ctx.memory_usage()["packed_staging"] == 0
        assert ctx.rgb_scratch_bytes() == 0
    finally:
        ctx.close()


def test_entropy_input_grows(pkg, monkeypatch):
    """The device's entropy decoder: one frame, then all ten -- status and scratch grow between two launches, and each of the two
    input sets is allocated --, then all ten once more, which grows the first set behind the launch that read it."""
    monkeypatch.delenv("VP8HIP_RECON", raising=False)
    P = pkg
    name = "kf_640x360"
    w, h, frames = P.read_ivf(ivf_path(name))
    parser = P.Parser()
    efs = []
    for data in frames:
        hdr, _ = parser.begin(data)
        efs.append(parser.export_entropy())
        parser.swap(hdr)
    parser.close()
    n = len(frames)
    ctx = P.Vp8Hip(0)
    try:
        ctx.configure(w, h, n, n)
        assert not ctx.entropy_decode(0, efs[:1], frames[:1]).any()
        assert not ctx.entropy_decode(0, efs, frames).any()
        assert not ctx.entropy_decode(0, efs, frames).any()
        ctx.decode([(i, i, None) for i in range(n)])
        assert ctx.frames_md5(0, n) == golden_md5(name)
    finally:
        ctx.close()
