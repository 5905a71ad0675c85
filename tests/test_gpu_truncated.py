"""GPU: frames whose token partition stops short.  The reference decodes on: from the macroblock at which its bool decoder
reports the end of data (vp8dx_bool_error, vp8/decoder/dboolhuff.h:131-153) no tokens are read, the macroblocks keep their
parsed skip flag -- so their inner edges are still loop-filtered -- and get no residual (decode_macroblock,
vp8/decoder/decodframe.c:119-130), and the frame is flagged corrupt.  The product's feeder has to switch over at the same
macroblock: its decode_to_md5 listing of damaged streams equals the one the reference decoder prints for the same file --
oracle/_ref/ref_md5 where the reference is built here (oracle/Makefile), else what it printed for a file with the same SHA-256
(tests/golden/truncated_ref_md5.json; VP8_RECORD_REF_DIGESTS=1 with the reference built rewrites it)."""
import hashlib
import json
import os
import struct
import subprocess

import pytest

from vp8_testlib import GOLDEN, ROOT, ivf_path

pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "libvpx.opencl_amd", "bin", "decode_to_md5")
REF = os.path.join(ROOT, "oracle", "_ref", "ref_md5")
LISTINGS = os.path.join(GOLDEN, "truncated_ref_md5.json")
RECORD = os.environ.get("VP8_RECORD_REF_DIGESTS") == "1"


def damaged(src, dst, victim, cut):
    """copy an IVF, dropping the last `cut` bytes of frame `victim`"""
    data = open(src, "rb").read()
    out = bytearray(data[:32])
    off, k = 32, 0
    while off + 12 <= len(data):
        size, = struct.unpack_from("<I", data, off)
        frame = data[off + 12: off + 12 + size]
        if k == victim:
            frame = frame[:len(frame) - cut]
        out += struct.pack("<I", len(frame)) + data[off + 4: off + 12] + frame
        off += 12 + size
        k += 1
    open(dst, "wb").write(out)


def reference_run(key, stream, want):
    """The reference decoder on a damaged stream: (decoded without error, reported a corrupt frame); its listing written to `want`.
    Live where oracle/_ref/ref_md5 is built (and then equal to the record), else the recorded run of the same bytes."""
    sha = hashlib.sha256(open(stream, "rb").read()).hexdigest()
    table = json.load(open(LISTINGS)) if os.path.exists(LISTINGS) else {}
    live = None
    if os.path.exists(REF):
        if os.path.exists(want):
            os.remove(want)
        r = subprocess.run([REF, str(stream), str(want)], capture_output=True, text=True)
        live = {"stream_sha256": sha, "ok": r.returncode == 0, "corrupt": "Corrupt frame detected" in r.stderr,
                "listing": open(want).read() if os.path.exists(want) else ""}
    if RECORD:
        assert live is not None, "VP8_RECORD_REF_DIGESTS=1 needs the reference build (make -C oracle ref)"
        table[key] = live
        with open(LISTINGS, "w") as f:
            json.dump(table, f, indent=1, sort_keys=True)
            f.write("\n")
    rec = table.get(key)
    assert rec is not None, f"{key}: no reference run recorded in {LISTINGS}"
    assert rec["stream_sha256"] == sha, f"{key}: the damaged stream is not the one the reference run was recorded from"
    if live is not None:
        assert live == rec, key
    open(want, "w").write(rec["listing"])
    return rec["ok"], rec["corrupt"]


@pytest.mark.parametrize("name,victim,cuts", [("kf_640x360", 1, (1, 7, 100, 1000, 9000)), ("p_1920x1080", 3, (3, 50, 250, 2000)),
                                              ("kf_odd_67x45", 0, (2, 30)), ("p_split_352x288", 2, (5, 200))])
def test_truncated_token_partition_like_the_reference(tmp_path, name, victim, cuts):
    for cut in cuts:
        bad = tmp_path / f"{name}_{victim}_{cut}.ivf"
        damaged(ivf_path(name), bad, victim, cut)
        want, got = tmp_path / "ref.md5", tmp_path / "hip.md5"
        ref_ok, ref_corrupt = reference_run(f"{name}_{victim}_{cut}", bad, want)
        g = subprocess.run([BIN, str(bad), str(got)], capture_output=True, text=True)
        # a cut that reaches into the first partition is an error in both (decodframe.c:733-736), after the same frames
        assert (g.returncode == 0) == ref_ok, (name, victim, cut, g.stderr)
        if not ref_ok:
            assert ref_corrupt and "Corrupt frame detected" in g.stderr, g.stderr
            assert len(open(want).read().splitlines()) == victim
        assert open(got).read() == open(want).read(), (name, victim, cut)
