"""CPU: the table of picture sizes tests/test_gpu_geometry.py decodes at (tests/vp8_testlib.py: WIDE_SIZES) stands where the rule
on LDS changes its answer -- so an edit to the table, or to the rule as DESIGN.md 5a states it, is noticed without a GPU."""
from vp8_testlib import RECON_LDS_LIMIT, TALL_SIZES, WIDE_SIZES, recon_lds_bytes, recon_waves_by_rule


def test_the_widths_stand_at_the_thresholds():
    for w, h, nw in WIDE_SIZES:
        assert recon_waves_by_rule(w, h) == nw, (w, h)
        assert nw // 2 < (h + 15) // 16 or nw == 2, (w, h, "the rule on rows would halve the count")
        assert ((w + 15) // 16) * ((h + 15) // 16) <= 3072
    assert {nw for _, _, nw in WIDE_SIZES} == {12, 10, 8, 6, 4, 2}
    # the last aligned width of every count, written out, and the first past it
    for nw, last in ((12, 2304), (10, 2976), (8, 4000), (6, 5696), (4, 9088)):
        assert recon_lds_bytes(nw, last) <= RECON_LDS_LIMIT < recon_lds_bytes(nw, last + 16), (nw, last)
        assert recon_waves_by_rule(last, 4096) == nw and recon_waves_by_rule(last + 16, 4096) == nw - 2, last
    assert recon_lds_bytes(12, 2304) == RECON_LDS_LIMIT            # (the widest picture with 12 waves fills a CU's LDS to the byte)
    assert recon_lds_bytes(2, 16384) <= RECON_LDS_LIMIT            # (no width vp8hip_configure accepts is refused for LDS)
    # every wide size is the first aligned width past a threshold or the last one before it, or the widest picture
    edges = {2304, 2304 + 16, 2976 + 16, 4000 + 16, 5696 + 16, 9088 + 16, 16384}
    assert {(w + 15) // 16 * 16 for w, _, _ in WIDE_SIZES} == edges


def test_the_tall_sizes():
    assert [((w + 15) // 16, (h + 15) // 16) for w, h in TALL_SIZES] == [(1, 1024), (3, 257), (3, 513)]
