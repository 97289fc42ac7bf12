"""The re-fit transcode targets, block by block, on a real MI355X: the checks of tests/test_hipemu_transcode_ref.py (byte equality with the
plain NumPy references of tests/transcode_ref.py for every block, the properties through the independent decoders, the coverage condition) on
the device build, plus the full-size cases: 2048^2 x 5 opaque and 2048^2 x 2 with alpha (ETC1S), 2048^2 x 1 (UASTC)."""
import numpy as np
import pytest

import transcode_cases as TC
from test_hipemu_transcode_ref import assert_coverage, check_case_table, check_etc1s_file, check_mixed_batch, check_uastc_file

pytestmark = pytest.mark.gpu


def test_gpu_transcode_case_table_blocks_equal_reference(oracle, gpu_codec):
    """The case table of the host-emulation test on the device: every block of every target, layers (a) and (b), every branch reached."""
    counters = {}
    check_case_table(oracle, gpu_codec, counters)
    assert_coverage(counters)


def test_gpu_transcode_mixed_batch(oracle, gpu_codec):
    check_mixed_batch(oracle, gpu_codec)


def test_gpu_transcode_full_size_etc1s(oracle, gpu_codec):
    """2048^2 x 5 opaque and 2048^2 x 2 with alpha: all 262,144 blocks of every layer of every target against the reference (computed per
    distinct source tuple and scattered: whole segments, nothing sampled).  The files are this codec's own (its encoder is pinned byte for
    byte elsewhere); what is judged is read from them by the pinned decoder."""
    counters = {}
    for name, n, alpha in (("2048x5", 5, False), ("2048x2_alpha", 2, True)):
        data = gpu_codec.encode_texture_segment(TC.sequence(n, 2048, 2048, 900 + n, alpha))
        d = check_etc1s_file(oracle, gpu_codec, name, data, counters)
        assert (d.width, d.height, max(1, d.layers), bool(d.has_alpha)) == (2048, 2048, n, alpha)


def test_gpu_transcode_full_size_uastc(oracle):
    """2048^2 x 1 UASTC with alpha: every block of ETC1, BC1 and BC3 against the reference.  ETC2 RGBA: every block of the border rows and
    columns plus a seeded sample of 16,384 interior blocks (the EAC search - 16 tables x 15 multipliers x 5 bases per distinct alpha block -
    is too slow in NumPy for a full layer of distinct blocks); its colour half is the ETC1 target's block, compared in full."""
    import uvol
    cu = uvol.Codec(device=0, uastc=1)
    try:
        data = cu.encode_texture_segment(TC.sequence(1, 2048, 2048, 950, True))
        check_uastc_file(oracle, cu, "2048x1 (uastc)", data, {}, sampled=("etc2_rgba",))
        (e1,), s1 = cu.transcode_texture_segments_status([data], "etc1"); (e2,), s2 = cu.transcode_texture_segments_status([data], "etc2_rgba")
        assert s1 == [0] and s2 == [0] and np.array_equal(e2[..., 8:], e1)
    finally:
        cu.close()
