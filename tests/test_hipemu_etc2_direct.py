"""The direct ETC2 RGB encode (uvol_encode_etc2_rgb_batch, csrc/tex_etc2.hip) through the host emulation of the kernels (tests/hipemu, no
GPU), and `uvolenc --etc2-direct` linked against the emulation library.  The checks are in tests/etc2_direct_cases.py;
tests/test_gpu_etc2_direct.py runs the same ones on the MI355X."""
import os
import subprocess
import numpy as np
import pytest
import etc2_direct_cases as EC
import material_cases as MC
from conftest import ROOT


@pytest.fixture()
def emu(hipemu_lib):
    import uvol
    cd = uvol.Codec(lib_path=hipemu_lib)
    yield cd
    cd.close()


@pytest.fixture(scope="module")
def emu_bins():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "universal-volumetric_amd"), "hipemu-bins"])
    return os.path.join(ROOT, "tests", "hipemu", "bin")


def test_etc2_direct_reference_properties():
    """CPU only: the NumPy restatement on the constructed content takes every branch of the rule, its blocks are never worse than the plain
    ETC1 fit and never leave the differential range; two worked blocks."""
    img, want, cnt = EC.constructed_reference()
    print(cnt)
    EC.check_properties(want, img)
    # a flat block of expand5(8, 16, 24): no modifier is zero, so base q leaves 3 x 2^2 per texel; the search moves the base one step up on
    # all channels (74, 140, 206), where table 0's -8 reaches the colour exactly: differential, zero deltas, error 0
    flat = np.empty((4, 4, 4), np.uint8); flat[:] = (66, 132, 198, 255)
    (blk,), _ = EC.reference("flat", [flat])
    assert blk[0, 0].tolist() == [9 << 3, 17 << 3, 25 << 3, 2, 0xFF, 0xFF, 0xFF, 0xFF] and EC.block_sse(blk, flat)[0].tolist() == [0]
    # left half black, right half white: individual (the q5 differ by 31), flip 0, each half reproduced up to the smallest modifier
    lr = np.zeros((4, 4, 4), np.uint8); lr[:, 2:] = 255
    (blk,), _ = EC.reference("left right", [lr], 0)
    assert blk[0, 0, :3].tolist() == [0x0F] * 3 and (blk[0, 0, 3] & 3) == 0 and EC.block_sse(blk, lr, 0)[0].tolist() == [0]


def test_hipemu_etc2_direct_bit_exact_shapes(emu):
    EC.run_shapes(emu, MC.HostMem())


def test_hipemu_etc2_direct_bit_exact_shapes_without_y_flip(hipemu_lib):
    import uvol
    cd = uvol.Codec(lib_path=hipemu_lib, y_flip=0)
    try:
        EC.run_shapes(cd, MC.HostMem(), y_flip=0)
    finally:
        cd.close()


def test_hipemu_etc2_direct_constructed_content(emu):
    EC.run_constructed(emu, MC.HostMem())


def test_hipemu_etc2_direct_against_the_transcoded_target(emu):
    EC.run_against_transcode(emu, MC.HostMem())


def test_hipemu_etc2_direct_sources_and_sinks(emu, hipemu_lib):
    import uvol
    from test_hipemu_tex import png_scanlines
    arena = uvol.PinnedArena(4096, lib_path=hipemu_lib)
    try:
        EC.run_sources_and_sinks(emu, MC.HostMem(), png_scanlines, arena)
    finally:
        arena.close()


def test_hipemu_etc2_direct_refusals_and_profile_group(emu):
    import uvol
    EC.run_refusals(emu, MC.HostMem(), uvol.UvolError)
    EC.run_profile_group(emu)


def test_uvolenc_hipemu_etc2_direct(emu_bins, tmp_path):
    EC.run_driver(os.path.join(emu_bins, "uvolenc"), str(tmp_path))


def test_uvolenc_hipemu_etc2_direct_uastc(emu_bins, tmp_path):
    EC.run_driver(os.path.join(emu_bins, "uvolenc"), str(tmp_path), uastc=True)
