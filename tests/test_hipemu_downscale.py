"""The device downscale (uvol_downscale_rgba_batch_dev, csrc/tex_downscale.hip) through the host emulation of the kernels (tests/hipemu, no
GPU), and `uvolenc --texture-ladder` linked against the emulation library.  The checks are in tests/downscale_cases.py; tests/test_gpu_downscale.py
runs the same ones on the MI355X."""
import os
import subprocess
import pytest
import downscale_cases as DC
import material_cases as MC
from conftest import GOLDEN, ROOT


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


def test_downscale_table_and_reference_properties():
    """CPU only: what the definition states about lin[], and its three worked examples through the NumPy restatement."""
    import numpy as np
    DC.check_table()
    chk = np.zeros((2, 2, 4), np.uint8); chk[..., 3] = 255; chk[0, 1, :3] = 255; chk[1, 0, :3] = 255
    assert DC.downscale(chk, 2)[0, 0].tolist() == [188, 188, 188, 255]
    tn = np.empty((2, 2, 4), np.uint8); tn[:] = (0, 255, 0, 0); tn[0, 0] = (200, 100, 50, 255)
    assert DC.downscale(tn, 2)[0, 0].tolist() == [200, 100, 50, 64]
    const = np.empty((5, 9, 4), np.uint8); const[:] = (3, 99, 250, 17)
    for f in DC.FACTORS:
        assert (DC.downscale(const, f) == const[0, 0]).all()
    assert DC.downscale(np.zeros((9, 17, 4), np.uint8), 8).shape == (2, 3, 4)


def test_hipemu_downscale_bit_exact_shapes(emu):
    DC.run_shapes(emu, MC.HostMem())


def test_hipemu_downscale_layers_of_an_ingest_slot(emu):
    from test_hipemu_tex import png_scanlines
    DC.run_ingest_slot(emu, MC.HostMem(), png_scanlines)


def test_hipemu_downscale_host_inputs(emu):
    DC.run_host_inputs(emu, MC.HostMem())


def test_hipemu_downscale_arithmetic_edges(emu):
    DC.run_arithmetic_edges(emu, MC.HostMem())


def test_hipemu_downscale_into_the_encoder(oracle, emu):
    DC.run_into_encoder(oracle, emu, MC.HostMem())


def test_hipemu_downscale_into_the_uastc_encoder(oracle, hipemu_lib):
    import uvol
    cu = uvol.Codec(lib_path=hipemu_lib, uastc=1)
    try:
        DC.run_into_encoder(oracle, cu, MC.HostMem(), uastc=True)
    finally:
        cu.close()


def test_hipemu_downscale_slots_trim_and_refusals(emu):
    import uvol
    DC.run_slots(emu, MC.HostMem())
    DC.run_refusals(emu, MC.HostMem(), uvol.UvolError)


def test_uvolenc_hipemu_texture_ladder(oracle, emu, emu_bins, tmp_path):
    DC.run_driver(oracle, os.path.join(emu_bins, "uvolenc"), str(tmp_path), emu.ktx2_info)


def test_uvolenc_hipemu_texture_ladder_host_images_and_uastc(oracle, emu, emu_bins, tmp_path):
    """The rungs from HOST images (--host-png-unfilter) are the rungs from device layers; with --uastc the rungs are UASTC files."""
    import cli_helpers
    exe = os.path.join(emu_bins, "uvolenc")
    for name, extra, enc in (("host", ["--host-png-unfilter"], oracle.ktx2_encode), ("uastc", ["--uastc"], oracle.uastc_ktx2_encode)):
        root = str(tmp_path / name); os.makedirs(root)
        cfgp, cfg, meshes, texs = cli_helpers.make_sequence(root, n_frames=5, tex=16, batch=3)
        r = subprocess.run([exe, cfgp, "--batch-frames", "3", "--texture-ladder", "2"] + extra, cwd=root, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout + r.stderr
        for s, n in enumerate([3, 2]):
            got = open(os.path.join(cfg["OutputDirectory"], "texture_ktx2_8x8_baseColor_default", "%05d.ktx2" % s), "rb").read()
            assert got == enc([DC.downscale(t, 2) for t in texs[3 * s:3 * s + n]]), (name, s)


def test_uvolenc_hipemu_without_the_new_flags_is_unchanged(emu_bins, tmp_path):
    got = DC.run_driver_default_unchanged(os.path.join(emu_bins, "uvolenc"), str(tmp_path))
    assert got == open(os.path.join(GOLDEN, "downscale_default_manifest.json"), "rb").read()
