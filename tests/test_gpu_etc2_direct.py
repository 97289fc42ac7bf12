"""The direct ETC2 RGB encode (uvol_encode_etc2_rgb_batch, csrc/tex_etc2.hip) on a real MI355X, through the C ABI, and `uvolenc --etc2-direct`
with the real binaries: the checks of tests/etc2_direct_cases.py (shared with tests/test_hipemu_etc2_direct.py)."""
import os
import pytest
import etc2_direct_cases as EC
import material_cases as MC
from conftest import ROOT

pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "universal-volumetric_amd", "bin")


def test_gpu_etc2_direct_bit_exact_shapes(gpu_codec):
    EC.run_shapes(gpu_codec, MC.HipMem())


def test_gpu_etc2_direct_bit_exact_shapes_without_y_flip():
    import uvol
    cd = uvol.Codec(device=0, y_flip=0)
    try:
        EC.run_shapes(cd, MC.HipMem(), y_flip=0)
    finally:
        cd.close()


def test_gpu_etc2_direct_more_blocks_than_one_round_of_the_grid(gpu_codec):
    EC.run_grid_stride(gpu_codec, MC.HipMem())


def test_gpu_etc2_direct_constructed_content(gpu_codec):
    EC.run_constructed(gpu_codec, MC.HipMem())


def test_gpu_etc2_direct_against_the_transcoded_target(gpu_codec):
    EC.run_against_transcode(gpu_codec, MC.HipMem())


def test_gpu_etc2_direct_sources_and_sinks(gpu_codec):
    import uvol
    from test_hipemu_tex import png_scanlines
    arena = uvol.PinnedArena(4096)
    try:
        EC.run_sources_and_sinks(gpu_codec, MC.HipMem(), png_scanlines, arena)
    finally:
        arena.close()


def test_gpu_etc2_direct_refusals_and_profile_group():
    import uvol
    cd = uvol.Codec(device=0)          # a context of its own: the profile switch is per context
    try:
        EC.run_refusals(cd, MC.HipMem(), uvol.UvolError)
        EC.run_profile_group(cd)
    finally:
        cd.close()


def test_gpu_uvolenc_etc2_direct(tmp_path):
    EC.run_driver(os.path.join(BIN, "uvolenc"), str(tmp_path))


def test_gpu_uvolenc_etc2_direct_uastc(tmp_path):
    EC.run_driver(os.path.join(BIN, "uvolenc"), str(tmp_path), uastc=True)
