"""CPU: streams that change their frame size in mid-stream (tests/stream_testlib.py: MAIN, MFQE, ALIGNED).  A key frame with a new
width or height makes the reference allocate everything again (vp8/decoder/decodframe.c:771-808 -> vp8_alloc_frame_buffers); here
the host feeder does (csrc/host/vp8_parser.c: resize) with state left over from the size before -- mode info, above contexts,
concealment arrays, the partition threads' progress array -- and the reference bookkeeping starts again.
 * the REFERENCE decoder's listing of each stream -- plain and through its post-processing -- equals feeder + oracle
   (+ OraclePostproc): oracle/_ref/ref_md5 where it is built, else its listing recorded for a stream with the same SHA-256
   (tests/golden/sizechange_ref.json; VP8_RECORD_REF_DIGESTS=1 with the reference built rewrites it);
 * the feeder reads back what was written, on 1 and 4 partition threads, dense and compact;
 * reference-buffer indices around every key frame; lost frames concealed after a reallocation;
 * what tests/test_gpu_sizechange.py needs of the reference beyond listings (its answers to the read-only controls, its vpxdec's
   digest) is recorded here as well."""
import os
import subprocess

import numpy as np
import pytest

import stream_testlib as S
from stream_testlib import (LISTINGS, assert_stream_covers, decode_with_oracle, mfqe_fires, recorded, reference_listing, section_starts,
                            size_changing, stream)



@pytest.fixture(scope="module")
def ivf_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("sizechange")


def test_the_streams_keep_their_point():
    for name, hidden in (("MAIN", 2), ("MFQE", 0), ("ALIGNED", 0)):
        sections, frames, expect = stream(name)
        assert_stream_covers(sections, expect, hidden)
    sections = stream("MAIN")[0]
    assert [s[:2] for s in sections] == [(48, 32), (176, 144), (67, 45), (67, 45), (80, 48), (70, 40), (16, 16), (130, 98), (48, 32),
                                         (16, 400), (1040, 16)]
    assert {s[4] for s in sections} == {0, 1, 2, 3}
    assert all(s[3][0] == "keep" for name in S.STREAMS for s in stream(name)[0])
    assert len(size_changing(sections)) == 10 and section_starts(sections)[3] not in size_changing(sections)
    # MFQE and ALIGNED: no key frame is above the frame shown before it -- MFQE cannot act on a frame that changes the size
    for name in ("MFQE", "ALIGNED"):
        sections, frames, expect = stream(name)
        last = None
        for i, (hdr, *_) in enumerate(expect):
            if hdr.frame_type == 0 and last is not None:
                assert hdr.base_qindex <= last, (name, i)
            if hdr.show_frame:
                last = hdr.base_qindex
        assert not set(mfqe_fires(frames)) & set(section_starts(sections)), name


@pytest.mark.parametrize("name,pp", LISTINGS, ids=[S.pp_key(n, pp) for n, pp in LISTINGS])
def test_reference_listing_equals_feeder_and_oracle(name, pp, ivf_dir):
    """Every listing here is the REFERENCE's: it survives all ten, the two ALIGNED configurations (MFQE with a deblocking filter,
    sizes that are multiples of 16) included."""
    ref = reference_listing(name, ivf_dir, pp)
    frames = stream(name)[1]
    if pp is None:
        assert decode_with_oracle(frames) == ref
        return
    mine, state = decode_with_oracle(frames, pp)
    assert mine == ref
    if pp[0] & 1024:
        assert state.mfqe_frames >= 6


def test_mfqe_on_a_frame_that_changes_the_size_is_not_pinned(ivf_dir):
    """MAIN with MFQE alone: its quantisers are the seeds', and MFQE does act on key frames that change the size.  There the
    reference blends the new picture with its freshly allocated post_proc_buffer -- whatever the allocator handed out --, so those
    frames have no defined value in the reference; the oracle (and the product) blend with zeros.  They are left out by index, the
    indices derived from the quantisers as read back; every other frame equals the reference's."""
    sections, frames, expect = stream("MAIN")
    pp = (1024, 0, 0)
    ref = reference_listing("MAIN", ivf_dir, pp)
    mine, state = decode_with_oracle(frames, pp)
    undefined = set(mfqe_fires(frames)) & set(size_changing(sections))
    assert undefined and len(undefined) <= len(size_changing(sections)) - 1
    assert all(expect[i][0].frame_type == 0 for i in undefined)
    assert state.mfqe_frames == len(mfqe_fires(frames))
    left_out = {"-%04d.i420" % (i + 1) for i in undefined}
    keep = lambda lines: [ln for ln in lines if ln[ln.rindex("-"):] not in left_out]
    assert len(ref) == len(mine) and [ln.split()[1] for ln in ref] == [ln.split()[1] for ln in mine]
    assert keep(mine) == keep(ref) and len(keep(ref)) == len(ref) - len(undefined)


HDR_FIELDS = ("width", "height", "mb_cols", "mb_rows", "frame_type", "show_frame", "filter_type", "filter_level", "sharpness_level",
              "segmentation_enabled", "base_qindex", "refresh_last", "refresh_golden", "refresh_alt", "copy_buffer_to_gf",
              "copy_buffer_to_arf", "sign_bias_golden", "sign_bias_alt", "num_token_partitions")


@pytest.mark.parametrize("name", ["MAIN", "ALIGNED"])
def test_feeder_reads_back_what_was_written(pkg, name):
    """As test_writer_cpu.test_feeder_reads_back_inter_frames asserts, over the changes of size (the size itself included); on
    one partition thread and on four -- clamped to the macroblock rows, which go down to one (16x16, 1040x16) -- with identical
    dense IR, and a compact IR that expands to it."""
    P = pkg
    sections, frames, expect = stream(name)
    parsers = {(t, form): P.Parser() for t in (1, 4) for form in ("dense", "compact")}
    for (t, _), p in parsers.items():
        p.set_threads(t)
    for k, (data, (hdr, mbs, coef, mvs)) in enumerate(zip(frames, expect)):
        h2, changed, m2, c2, v2 = P.parse_to_numpy(parsers[1, "dense"], data)
        parsers[1, "dense"].swap(h2)
        assert changed == (k in size_changing(sections)), k
        for f in HDR_FIELDS:
            if hdr.frame_type == 0 and f.startswith(("refresh", "copy", "sign")):
                continue
            assert getattr(h2, f) == getattr(hdr, f), (k, f)
        assert h2.segmentation_enabled == 1
        assert h2.mb_segment_abs_delta == hdr.mb_segment_abs_delta, k
        assert list(h2.segment_quant) == list(hdr.segment_quant) and list(h2.segment_lf) == list(hdr.segment_lf), k
        assert m2.shape == mbs.shape and np.array_equal(m2[:, 4], mbs[:, 4]), k        # (kept maps: the new key frame's)
        assert np.array_equal(m2[:, 0], mbs[:, 0]) and np.array_equal(m2[:, 2], mbs[:, 2]), k
        intra = mbs[:, 2] == 0
        assert np.array_equal(m2[intra, 1], mbs[intra, 1]), k
        bp = intra & (mbs[:, 0] == 4)
        assert np.array_equal(m2[bp, 40:56], mbs[bp, 40:56]), k
        assert np.array_equal(m2[:, 3] & 3, mbs[:, 3] & 3), k
        split = mbs[:, 0] == 9
        assert np.array_equal(m2[split, 5], mbs[split, 5]), k
        if hdr.frame_type:
            assert np.array_equal(v2, mvs), k
        live = (mbs[:, 3] & 1) == 0
        assert np.array_equal(m2[live, 8:33], mbs[live, 8:33]) and np.array_equal(c2[live], coef[live]), k
        # four threads, dense: byte for byte
        h4, ch4, m4, c4, v4 = P.parse_to_numpy(parsers[4, "dense"], data)
        parsers[4, "dense"].swap(h4)
        assert ch4 == changed and bytes(h4) == bytes(h2) and (m4 == m2).all() and (c4 == c2).all() and (v4 == v2).all(), k
        # compact, one thread and four: expands to the dense IR
        for t in (1, 4):
            hc, mbx, blocks, vc, corrupt = P.parse_to_numpy_compact(parsers[t, "compact"], data)
            parsers[t, "compact"].swap(hc)
            assert corrupt == 0 and (vc == v2).all(), (k, t)
            mc, cc = P.dense_from_compact(mbx, blocks)
            assert (mc == m2).all() and (cc[live] == c2[live]).all(), (k, t)
    for p in parsers.values():
        p.close()


def test_reference_bookkeeping_around_key_frames(pkg):
    """vp8_alloc_frame_buffers (alloccommon.c:87-95): after a key frame of a new size new, last, golden, alt-ref are buffers
    0, 1, 2, 3, and once it is swapped in all three references are the new frame; a key frame of the size before takes a free
    buffer like any frame and resets nothing."""
    P = pkg
    sections, frames, _ = stream("MAIN")
    starts, changing = section_starts(sections), size_changing(sections)
    parser = P.Parser()
    for k, data in enumerate(frames):
        before = (parser.refs.lst_idx, parser.refs.gld_idx, parser.refs.alt_idx)
        hdr, changed, *_ = P.parse_to_numpy(parser, data)
        r = parser.refs
        if k in changing:
            assert changed and (r.new_idx, r.lst_idx, r.gld_idx, r.alt_idx) == (0, 1, 2, 3) and list(r.ref_cnt) == [1, 1, 1, 1], k
        else:
            assert not changed and (r.lst_idx, r.gld_idx, r.alt_idx) == before and r.new_idx not in before, k
        new = r.new_idx
        parser.swap(hdr)
        if k in starts:
            assert (r.lst_idx, r.gld_idx, r.alt_idx, r.show_idx) == (new,) * 4 and r.ref_cnt[new] == 3 and sum(r.ref_cnt) == 3, k
    parser.close()


def test_begin_again_after_abandoning_a_frame_of_a_new_size(pkg):
    """What Vp8Hip.parse_into_slot does when the context has another size: Parser.begin, Parser.abandon, and -- once the context is
    configured -- begin on the same frame again.  The second begin reports the change again and finds the bookkeeping as the first
    did (it used to fail with "no free frame buffer": begin had taken all four buffers, and nothing gave the new one back)."""
    P = pkg
    sections, frames, _ = stream("MAIN")
    at = section_starts(sections)[1]
    parser = P.Parser()
    for data in frames[:at]:
        hdr, *_ = P.parse_to_numpy(parser, data)
        parser.swap(hdr)
    state = bytes(parser.refs), parser.dims
    hdr, changed = parser.begin(frames[at])
    assert changed and (hdr.width, hdr.height) == (176, 144) and parser.dims == (176, 144)
    parser.abandon()
    assert (bytes(parser.refs), parser.dims) == state
    parser.abandon()                                    # (nothing left to undo)
    assert (bytes(parser.refs), parser.dims) == state
    again = P.Parser()
    hdr, changed, mbs, coef, mvs = P.parse_to_numpy(parser, frames[at])
    r = parser.refs
    assert changed and (r.new_idx, r.lst_idx, r.gld_idx, r.alt_idx) == (0, 1, 2, 3)
    parser.swap(hdr)
    # ... and the section reads as it does on a parser that never abandoned anything
    for data in frames[:at + 1]:
        h0, *_ = P.parse_to_numpy(again, data)
        again.swap(h0)
    for data in frames[at + 1:section_starts(sections)[2]]:
        a, b = P.parse_to_numpy(parser, data), P.parse_to_numpy(again, data)
        parser.swap(a[0]); again.swap(b[0])
        assert bytes(a[0]) == bytes(b[0]) and all((x == y).all() for x, y in zip(a[2:], b[2:]))
        assert bytes(parser.refs) == bytes(again.refs)
    # an inter frame abandoned: its buffer is free again
    state = bytes(parser.refs), parser.dims
    nxt = frames[section_starts(sections)[2] - 1]
    parser.begin(nxt)
    assert bytes(parser.refs) != state[0]
    parser.abandon()
    assert (bytes(parser.refs), parser.dims) == state
    parser.close(); again.close()


@pytest.mark.parametrize("section", [1, 2], ids=["176x144", "67x45"])
def test_lost_frame_concealed_after_a_reallocation(section, ivf_dir):
    """The reference configured --enable-error-concealment (oracle/_ref/ref_md5_ec --damage --ec --lose K) with the second inter
    frame of a section lost: concealment works from the mode info of the frame before and from overlap lists, both of which
    resize() allocated again for this size."""
    sections, frames, _ = stream("MAIN")
    k = section_starts(sections)[section] + 3                  # 1-based packet number of the section's second inter frame
    ivf = S.stream_ivf("MAIN", ivf_dir)
    ref = recorded("MAIN-ec-lose_%d" % k, ivf, lambda: S.run_ref_md5(ivf, ("--damage", "--ec", "--lose", k), tool=S.REF_MD5_EC))
    assert decode_with_oracle(frames, lose={k}) == ref
    assert ref != reference_listing("MAIN", ivf_dir)            # (the loss shows)


def test_reference_controls_are_what_the_headers_say(pkg, ivf_dir):
    """The reference's answers to VP8D_GET_LAST_REF_UPDATES / _USED / VP8D_GET_FRAME_CORRUPTED packet by packet (recorded here for
    tests/test_gpu_sizechange.py, from oracle/_ref/libvpxref.so): updates are the refresh flags -- all three on a key frame --,
    the references used are those of the macroblocks read back, and nothing is corrupt."""
    sections, frames, expect = stream("MAIN")
    ivf = S.stream_ivf("MAIN", ivf_dir)
    ref = recorded("MAIN-refctl", ivf, lambda: S.reference_controls(ivf), what="controls")
    assert len(ref) == len(frames)
    for k, ((hdr, mbs, _, _), (updates, used, corrupted)) in enumerate(zip(expect, ref)):
        if hdr.frame_type == 0:
            assert (updates, used) == (7, 0), k
        else:
            assert updates == hdr.refresh_last | hdr.refresh_golden << 1 | hdr.refresh_alt << 2, k
            assert used == sum(1 << (r - 1) for r in set(mbs[:, 2].tolist()) if r), k
        assert corrupted == 0, k


def test_reference_vpxdec_digest_is_the_listings(pkg, ivf_dir):
    """`vpxdec_ref --md5 --i420` (recorded here for tests/test_gpu_sizechange.py): one digest over all shown frames, each in its own
    size -- the MD5 of the oracle's frames one after the other."""
    import hashlib
    from vp8_testlib import oracle_frames
    ivf = S.stream_ivf("MAIN", ivf_dir)

    def live():
        if not os.path.exists(S.REF_VPXDEC):
            return None
        r = subprocess.run([S.REF_VPXDEC, "--md5", "--i420", ivf], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return r.stdout.split()[0]
    ref = recorded("MAIN-vpxdec_md5", ivf, live, what="digest")
    m = hashlib.md5()
    for hdr, changed, mbs, coef, mvs, new, shown in oracle_frames(stream("MAIN")[1]):
        if shown is not None:
            w, h = hdr.width, hdr.height
            g = pkg.geom(w, h)
            for off, stride, pw, ph in ((g.y_off, g.y_stride, w, h), (g.u_off, g.uv_stride, (w + 1) // 2, (h + 1) // 2),
                                        (g.v_off, g.uv_stride, (w + 1) // 2, (h + 1) // 2)):
                m.update(np.ascontiguousarray(np.lib.stride_tricks.as_strided(shown[off:], shape=(ph, pw), strides=(stride, 1))).tobytes())
    assert m.hexdigest() == ref


def test_key_frame_with_a_zeroed_width_leaves_the_feeder_alone(pkg):
    """A copy of a section's key frame with its width bytes zeroed, after the key frame itself: the feeder refuses it before it
    allocates anything, gives the frame buffer back, and reads the section's inter frames as if nothing had happened."""
    P = pkg
    sections, frames, expect = stream("MAIN")
    starts = section_starts(sections)
    parser = P.Parser()
    for k, (data, (hdr, mbs, coef, mvs)) in enumerate(zip(frames[:starts[3]], expect)):
        h2, changed, m2, c2, v2 = P.parse_to_numpy(parser, data)
        parser.swap(h2)
        assert (m2[:, :6] == mbs[:, :6]).all() and (v2 == mvs).all(), k
        if k in starts:
            held = lambda r: (r.lst_idx, r.gld_idx, r.alt_idx, list(r.ref_cnt))      # (new_idx is whatever was tried last)
            state = held(parser.refs), parser.dims
            bad = bytearray(data)
            bad[6] = bad[7] = 0
            with pytest.raises(ValueError, match="Invalid frame width"):
                parser.begin(bytes(bad))
            assert (held(parser.refs), parser.dims) == state, k
    parser.close()
