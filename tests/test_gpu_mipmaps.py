"""Mip levels inside one UASTC .ktx2 (uvol_mipchain_rgba_batch_dev, uvol_encode_texture_segments_mips, uvol_transcode_texture_segments_level)
on a real MI355X, through the C ABI, and `uvolenc --mipmaps` / the basisu shim with the real binaries: the checks of tests/mipmap_cases.py
(shared with tests/test_hipemu_mipmaps.py)."""
import os
import pytest
import mipmap_cases as MM
import material_cases as MC
from conftest import ROOT

pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "universal-volumetric_amd", "bin")


@pytest.fixture(scope="module")
def gpu_uastc():
    import uvol
    cu = uvol.Codec(device=0, uastc=1)
    yield cu
    cu.close()


@pytest.fixture(scope="module")
def mip_files(oracle, gpu_uastc, gpu_codec):
    """The two 7-level files of the encode check, made once for the read checks."""
    import uvol
    return MM.run_encode(oracle, gpu_uastc, MC.HipMem(), uvol.UvolError, gpu_codec)


def test_gpu_mipchain_bit_exact_shapes(gpu_codec):
    MM.run_shapes(gpu_codec, MC.HipMem())


def test_gpu_mipchain_layer_at_a_4_byte_aligned_address(gpu_codec):
    MM.run_misaligned_layer(gpu_codec, MC.HipMem())


def test_gpu_mipchain_host_inputs(gpu_codec):
    MM.run_host_inputs(gpu_codec, MC.HipMem())


def test_gpu_mipchain_layers_of_an_ingest_slot(gpu_codec):
    from test_hipemu_tex import png_scanlines
    MM.run_ingest_slot(gpu_codec, MC.HipMem(), png_scanlines)


def test_gpu_mipchain_arithmetic_edges(gpu_codec):
    MM.run_arithmetic_edges(gpu_codec, MC.HipMem())


def test_gpu_mipchain_slots_trim_and_refusals():
    import uvol
    cd = uvol.Codec(device=0)          # a context of its own: uvol_trim gives back workspaces the shared context's other tests hold
    try:
        MM.run_slots(cd, MC.HipMem())
        MM.run_refusals(cd, MC.HipMem(), uvol.UvolError)
    finally:
        cd.close()


def test_gpu_encode_mips_byte_pin(mip_files):
    assert len(mip_files) == 2          # (the checks ran in the fixture, whose files the read tests share)


def test_gpu_read_levels(oracle, gpu_uastc, mip_files):
    MM.run_read(oracle, gpu_uastc, mip_files)


def test_gpu_read_levels_zstandard(oracle, gpu_uastc, mip_files):
    if MM.run_read_zstd(oracle, gpu_uastc, mip_files) is None:
        pytest.skip("libzstd.so.1 is not installed")


def test_gpu_uvolenc_mipmaps_and_basisu_shim(oracle, gpu_uastc, tmp_path):
    MM.run_driver(oracle, gpu_uastc, BIN, str(tmp_path))
