"""Mip levels inside one UASTC .ktx2 (uvol_mipchain_rgba_batch_dev, uvol_encode_texture_segments_mips, uvol_transcode_texture_segments_level)
through the host emulation of the kernels (tests/hipemu, no GPU), the container read by the reference's KTX-Parse, and `uvolenc --mipmaps` /
the basisu shim linked against the emulation library.  The checks are in tests/mipmap_cases.py; tests/test_gpu_mipmaps.py runs the same ones
on the MI355X."""
import os
import shutil
import subprocess
import pytest
import mipmap_cases as MM
import material_cases as MC
from conftest import ROOT


@pytest.fixture()
def emu(hipemu_lib):
    import uvol
    cd = uvol.Codec(lib_path=hipemu_lib)
    yield cd
    cd.close()


@pytest.fixture(scope="module")
def emu_uastc(hipemu_lib):
    import uvol
    cu = uvol.Codec(lib_path=hipemu_lib, uastc=1)
    yield cu
    cu.close()


@pytest.fixture(scope="module")
def mip_files(oracle, emu_uastc, hipemu_lib):
    """The two 7-level files of the encode check, made once for the read checks."""
    import uvol
    ce = uvol.Codec(lib_path=hipemu_lib)
    try:
        return MM.run_encode(oracle, emu_uastc, MC.HostMem(), uvol.UvolError, ce)
    finally:
        ce.close()


@pytest.fixture(scope="module")
def emu_bins():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "universal-volumetric_amd"), "hipemu-bins"])
    return os.path.join(ROOT, "tests", "hipemu", "bin")


def test_mip_restatement_equals_the_downscale_up_to_level_3():
    MM.check_restatement()


def test_hipemu_mipchain_bit_exact_shapes(emu):
    MM.run_shapes(emu, MC.HostMem())


def test_hipemu_mipchain_layer_at_a_4_byte_aligned_address(emu):
    MM.run_misaligned_layer(emu, MC.HostMem())


def test_hipemu_mipchain_host_inputs(emu):
    MM.run_host_inputs(emu, MC.HostMem())


def test_hipemu_mipchain_layers_of_an_ingest_slot(emu):
    from test_hipemu_tex import png_scanlines
    MM.run_ingest_slot(emu, MC.HostMem(), png_scanlines)


def test_hipemu_mipchain_arithmetic_edges(emu):
    MM.run_arithmetic_edges(emu, MC.HostMem())


def test_hipemu_mipchain_slots_trim_and_refusals(emu):
    import uvol
    MM.run_slots(emu, MC.HostMem())
    MM.run_refusals(emu, MC.HostMem(), uvol.UvolError)


def test_hipemu_encode_mips_byte_pin(mip_files):
    assert len(mip_files) == 2          # (the checks ran in the fixture, whose files the read tests share)


def test_hipemu_read_levels(oracle, emu_uastc, mip_files):
    MM.run_read(oracle, emu_uastc, mip_files)


def test_hipemu_read_levels_zstandard(oracle, emu_uastc, mip_files):
    if MM.run_read_zstd(oracle, emu_uastc, mip_files) is None:
        pytest.skip("libzstd.so.1 is not installed")


def test_mip_container_read_by_ktx_parse(oracle, emu_uastc, tmp_path):
    node = shutil.which("node")
    ref = "/root/reference/src/lib/ktx-parse.module.js"
    if not node or not os.path.exists(ref):
        pytest.skip("node or the reference's ktx-parse.module.js is absent")
    MM.run_ktx_parse(oracle, emu_uastc, tmp_path, node, ref)


def test_uvolenc_hipemu_mipmaps_and_basisu_shim(oracle, emu_uastc, emu_bins, tmp_path):
    MM.run_driver(oracle, emu_uastc, emu_bins, str(tmp_path))
