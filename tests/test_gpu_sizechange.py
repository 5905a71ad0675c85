"""GPU (-m gpu): streams that change their frame size in mid-stream (tests/stream_testlib.py: MAIN, MFQE, ALIGNED) through every way
into the product -- the vpx_codec API (csrc/host/vp8_dx_iface.c reconfigures a live context: a new pool, a new pinned frame, the
reference bookkeeping from the start, the post-processing state kept), the command line tools, the Python wrapper -- against the
REFERENCE decoder's listings (tests/golden/sizechange_ref.json, which tests/test_sizechange_cpu.py records and pins to feeder +
oracle), and the refusals of the paths that take one size only (batch_md5, vp8hip_entropy_decode).  All frames are tiny."""
import ctypes
import hashlib
import os
import subprocess

import pytest

import stream_testlib as S
from stream_testlib import (LISTINGS, Decoder, VpxRefFrame, codec_listing, decode_with_oracle, image_md5, image_plane, listing_line, mfqe_fires,
                            reference_listing, section_starts, size_changing, stream)
from vp8_testlib import ROOT, load_package
from vp8_writer import write_ivf

pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "libvpx.opencl_amd", "bin")


@pytest.fixture(scope="module")
def ivf_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("sizechange_gpu")


@pytest.fixture(scope="module")
def main_listing(ivf_dir):
    return reference_listing("MAIN", ivf_dir)


def _by_packet(listing):
    """{1-based packet number: line}"""
    return {int(ln[ln.rindex("-") + 1:ln.rindex(".")]): ln for ln in listing}


# ---- the vpx_codec API
@pytest.mark.parametrize("recon", [None, "simt"])
def test_codec_api_decodes_through_the_changes(recon, main_listing, monkeypatch):
    """Packet by packet, with both kernel families: every image is the reference's, has the frame's size, and its planes can be read
    to the last row.  vpx_codec_get_stream_info keeps answering the FIRST key frame's size, as the reference's does
    (vp8/vp8_dx_iface.c:364 peeks only while it has none)."""
    if recon:
        monkeypatch.setenv("VP8HIP_RECON", recon)
    else:
        monkeypatch.delenv("VP8HIP_RECON", raising=False)
    sections, frames, expect = stream("MAIN")
    want = _by_packet(main_listing)
    d = Decoder()
    for k, (data, (hdr, *_)) in enumerate(zip(frames, expect), 1):
        rc, img = d.decode(data)
        assert rc == 0, k
        assert (img is not None) == bool(hdr.show_frame) == (k in want), k
        if hdr.frame_type == 0:
            size = (hdr.width, hdr.height)
        if img is not None:
            assert (img.d_w, img.d_h) == size and img.stride[0] >= img.d_w and img.stride[1] >= (img.d_w + 1) // 2, k
            assert listing_line(image_md5(img), img.d_w, img.d_h, k) == want[k], k
        assert d.stream_info() == sections[0][:2], k
    d.close()


@pytest.mark.parametrize("name,pp", LISTINGS[1:], ids=[S.pp_key(n, pp) for n, pp in LISTINGS[1:]])
def test_codec_api_postproc_through_the_changes(name, pp, ivf_dir):
    """VPX_CODEC_USE_POSTPROC: the noise table, the last quantisers and the per-row phases stay in step across heights (the
    post-processing state outlives the reconfiguration, vp8hip_ctx.hip.h), while FB_POST / FB_PPINT / FB_PPTMP come new."""
    assert codec_listing(stream(name)[1], S.VPX_CODEC_USE_POSTPROC, pp) == reference_listing(name, ivf_dir, pp)


def test_codec_api_mfqe_on_frames_that_change_the_size(ivf_dir):
    """MAIN with MFQE alone: every frame against the ORACLE, the key frames included that change the size and on which MFQE acts
    (the reference has no defined value there: tests/test_sizechange_cpu.py).  Product and oracle both blend with zeros there: the
    raster pool is zero-filled when it is allocated (vp8hip_raster_pool), as is the oracle's buffer."""
    sections, frames, _ = stream("MAIN")
    pp = (1024, 0, 0)
    mine, state = decode_with_oracle(frames, pp)
    assert set(mfqe_fires(frames)) & set(size_changing(sections)) and state.mfqe_frames >= 6
    assert codec_listing(frames, S.VPX_CODEC_USE_POSTPROC, pp) == mine


def test_read_only_controls_answer_like_the_reference(ivf_dir):
    sections, frames, _ = stream("MAIN")
    ivf = S.stream_ivf("MAIN", ivf_dir)
    want = S.recorded("MAIN-refctl", ivf, lambda: None, what="controls")
    d = Decoder()
    for k, data in enumerate(frames):
        assert d.decode(data)[0] == 0, k
        got = [d.get_int(c) for c in (S.VP8D_GET_LAST_REF_UPDATES, S.VP8D_GET_LAST_REF_USED, S.VP8D_GET_FRAME_CORRUPTED)]
        assert got == want[k], k
    d.close()


def test_copy_and_set_reference_right_after_a_change(main_listing):
    """After the key frames that bring 176x144 (frame buffers of 176x144, after 48x32) and 67x45 (80x48, after 176x144): an image
    of the aligned size before is refused, one of the new aligned size is accepted and is the frame just shown; LAST set to its own
    content (a new buffer, borders extended on the host) leaves the rest of the stream bit-exact."""
    sections, frames, expect = stream("MAIN")
    want = _by_packet(main_listing)
    starts = section_starts(sections)
    at = {starts[1]: ((48, 32), (176, 144)), starts[2]: ((176, 144), (80, 48))}
    d = Decoder()
    L = d.L
    for k, data in enumerate(frames):
        rc, img = d.decode(data)
        assert rc == 0, k
        if img is not None:
            assert listing_line(image_md5(img), img.d_w, img.d_h, k + 1) == want[k + 1], k
        if k in at:
            old, new = at[k]
            w, h = img.d_w, img.d_h
            bad = VpxRefFrame()
            bad.frame_type = S.VP8_LAST_FRAME
            assert L.vpx_img_alloc(ctypes.byref(bad.img), S.VPX_IMG_FMT_I420, old[0], old[1], 1)
            assert d.control(S.VP8_COPY_REFERENCE, bad) != 0 and d.control(S.VP8_SET_REFERENCE, bad) != 0, k
            L.vpx_img_free(ctypes.byref(bad.img))
            for which in (S.VP8_LAST_FRAME, S.VP8_GOLD_FRAME, S.VP8_ALTR_FRAME):        # (a key frame: all three are the new frame)
                ref = VpxRefFrame()
                ref.frame_type = which
                assert L.vpx_img_alloc(ctypes.byref(ref.img), S.VPX_IMG_FMT_I420, new[0], new[1], 1)
                assert d.control(S.VP8_COPY_REFERENCE, ref) == 0, (k, which)
                assert image_plane(ref.img, 0, w, h) == image_plane(img, 0, w, h), (k, which)
                for p in (1, 2):
                    assert image_plane(ref.img, p, (w + 1) // 2, (h + 1) // 2) == image_plane(img, p, (w + 1) // 2, (h + 1) // 2), (k, which)
                if which == S.VP8_LAST_FRAME:
                    assert d.control(S.VP8_SET_REFERENCE, ref) == 0, k
                L.vpx_img_free(ctypes.byref(ref.img))
    d.close()


def test_key_frame_with_a_zeroed_width_changes_nothing(main_listing):
    """A copy of a section's key frame with its width bytes zeroed, sent after the key frame itself: vpx_codec_decode fails, and the
    section's inter frames -- on references nothing has touched, in a context nothing has reconfigured -- still decode to their
    listing entries.  (The product's behaviour; the reference's is not asked.)"""
    sections, frames, _ = stream("MAIN")
    want = _by_packet(main_listing)
    starts = section_starts(sections)
    d = Decoder()
    for k, data in enumerate(frames):
        rc, img = d.decode(data)
        assert rc == 0, k
        if img is not None:
            assert listing_line(image_md5(img), img.d_w, img.d_h, k + 1) == want[k + 1], k
        if k in (starts[1], starts[3], starts[6]):
            bad = bytearray(data)
            bad[6] = bad[7] = 0
            rc, img = d.decode(bytes(bad))
            assert rc != 0 and img is None, k
    d.close()


# ---- the command line tools
def test_tools_on_the_stream(main_listing, ivf_dir, tmp_path):
    P = load_package()
    sections, frames, expect = stream("MAIN")
    ivf = S.stream_ivf("MAIN", ivf_dir)
    out = tmp_path / "out.md5"
    r = subprocess.run([os.path.join(BIN, "decode_to_md5"), ivf, str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert open(out).read() == "".join(ln + "\n" for ln in main_listing)
    digest = S.recorded("MAIN-vpxdec_md5", ivf, lambda: None, what="digest")
    tools = [[os.path.join(BIN, "vpxdec")], [os.path.join(BIN, "vpxdec"), "--threads", "4"]]
    ref_on_hip = os.path.join(S.REFDIR, "vpxdec_ref_on_hip")
    if os.path.exists(ref_on_hip):
        tools.append([ref_on_hip])
    for tool in tools:
        r = subprocess.run(tool + ["--md5", "--i420", ivf], capture_output=True, text=True)
        assert r.returncode == 0, (tool, r.stderr)
        assert r.stdout.split()[0] == digest, tool
    raw = tmp_path / "o.i420"
    r = subprocess.run([os.path.join(BIN, "vpxdec"), "--i420", "-o", str(raw), ivf], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    size, data = 0, open(raw, "rb").read()
    for hdr, *_ in expect:
        if hdr.frame_type == 0:
            w, h = hdr.width, hdr.height
        if hdr.show_frame:
            size += P.i420_size(w, h)
    assert len(data) == size and hashlib.md5(data).hexdigest() == digest


# ---- the Python wrapper
def test_decode_ivf_gpu_reconfigures(main_listing, ivf_dir):
    P = load_package()
    assert P.decode_ivf_gpu(S.stream_ivf("MAIN", ivf_dir), device=0) == [ln.split()[0] for ln in main_listing]


@pytest.mark.parametrize("form", ["dense", "compact"])
def test_parse_into_slot_asks_for_a_reconfiguration_and_then_works(form, main_listing):
    """Vp8Hip.parse_into_slot / parse_into_slot_compact on a key frame of a new size raise; after ctx.configure(new size) the same
    call on the SAME parser succeeds (it used to fail with "no free frame buffer"), and the stream decodes to the listing."""
    P = load_package()
    sections, frames, _ = stream("MAIN")
    want = _by_packet(main_listing)
    changing = size_changing(sections)
    parser, ctx = P.Parser(), P.Vp8Hip(0)
    ctx.configure(sections[0][0], sections[0][1], 4, 1)

    def parse(data):
        if form == "dense":
            hdr = ctx.parse_into_slot(parser, data, 0)
            ctx.upload(0)
            return hdr
        return ctx.parse_into_slot_compact(parser, data, 0)[0]
    try:
        raised = 0
        for k, data in enumerate(frames):
            try:
                hdr = parse(data)
                assert k == 0 or k not in changing
            except RuntimeError as e:
                assert "reconfigure the context first" in str(e) and k in changing, (k, e)
                raised += 1
                w, h = sections[section_starts(sections).index(k)][:2]
                ctx.configure(w, h, 4, 1)
                hdr = parse(data)
                r = parser.refs
                assert (r.new_idx, r.lst_idx, r.gld_idx, r.alt_idx) == (0, 1, 2, 3)
            r = parser.refs
            ctx.decode([(0, r.new_idx, (r.lst_idx, r.gld_idx, r.alt_idx))])
            parser.swap(hdr)
            if hdr.show_frame:
                assert listing_line(P.planes_md5(*ctx.download_planes(parser.refs.show_idx)), ctx.width, ctx.height, k + 1) == want[k + 1], k
            else:
                ctx.sync()
        assert raised == len(changing) - 1
    finally:
        ctx.close()
        parser.close()


# ---- the paths that take one size refuse a second one
@pytest.mark.parametrize("args", [["--threads", "3"], ["--device-entropy"], ["--streams", "2"]], ids=["threads", "device-entropy", "streams"])
def test_batch_md5_refuses_a_second_size(args, tmp_path):
    sections, frames, _ = stream("MAIN")
    keys = [frames[k] for k in section_starts(sections)]
    ivf, out = tmp_path / "keys.ivf", tmp_path / "out.md5"
    write_ivf(ivf, sections[0][0], sections[0][1], keys)
    r = subprocess.run([os.path.join(BIN, "batch_md5")] + args + [str(ivf), str(out)], capture_output=True, text=True)
    assert r.returncode != 0 and r.stderr.strip(), (r.returncode, r.stderr)
    if os.path.exists(out):               # (the second frame has the second size: a listing may hold the first frame, no more)
        assert len(open(out).read().splitlines()) <= 1


def test_entropy_decode_refuses_another_size(main_listing):
    """vp8hip_entropy_decode in a context configured for 80x48: a 176x144 key frame is refused, and so is a 67x45 one -- the same
    5x3 macroblocks, another display size, by which the context's digests, downloads and tensors crop.  Neither touches the slot
    or the block pool."""
    P = load_package()
    sections, frames, _ = stream("MAIN")
    starts = section_starts(sections)
    want = _by_packet(main_listing)

    def exported(k):
        p = P.Parser()
        p.begin(frames[k])
        ef = p.export_entropy()
        p.close()
        assert ef is not None
        return ef
    ctx = P.Vp8Hip(0)
    try:
        w, h = 80, 48
        ctx.configure_pooled(w, h, 1, 1, 15 * 24 * 32 + 4 * 4 * 5 * 24 * 32)
        k = starts[4]
        assert sections[4][:2] == (w, h)
        ctx.pool_reset()
        assert not ctx.entropy_decode(0, [exported(k)], [frames[k]]).any()
        used = ctx.pool_usage()
        mbs, coef = ctx.ir_fetch(0)
        for other in (starts[1], starts[2], starts[5]):                  # 176x144; 67x45 and 70x40: the same 5x3 grid
            with pytest.raises(RuntimeError, match="context configured for"):
                ctx.entropy_decode(0, [exported(other)], [frames[other]])
            assert ctx.pool_usage() == used
            m2, c2 = ctx.ir_fetch(0)
            assert (m2 == mbs).all() and (c2 == coef).all()
        ctx.decode([(0, 0, None)])
        assert listing_line(ctx.frames_md5(0, 1)[0], w, h, k + 1) == want[k + 1]
    finally:
        ctx.close()
