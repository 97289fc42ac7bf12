"""The JPEG ingest (uvol_idct_jpeg_batch_dev, csrc/jpeg_ingest.hip) on a real MI355X, through the C ABI, and `uvolenc` / the `basisu` shim with
the real binaries: the device checks of tests/jpeg_cases.py (shared with tests/test_hipemu_jpeg.py, which also holds the CPU-only ones)."""
import os
import numpy as np
import pytest
import jpeg_cases as JC
import material_cases as MC
from conftest import ROOT

pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "universal-volumetric_amd", "bin")


@pytest.fixture(scope="module")
def host():
    return JC.hostlib()


def test_gpu_jpeg_fixtures_bit_exact(gpu_codec, host):
    JC.run_device_fixtures(gpu_codec, MC.HipMem(), host)


def test_gpu_jpeg_batch_of_five_both_slots(gpu_codec):
    JC.run_device_batch(gpu_codec, MC.HipMem())


def test_gpu_jpeg_inputs_in_host_alloc_memory(gpu_codec, host):
    import uvol
    arena = uvol.PinnedArena(1 << 20)
    try:
        JC.run_device_fixtures(gpu_codec, MC.HipMem(), host, arena=arena)
        JC.run_device_batch(gpu_codec, MC.HipMem(), arena=arena)
    finally:
        arena.close()


def test_gpu_jpeg_arithmetic_edges(gpu_codec):
    JC.run_arithmetic_edges(gpu_codec, MC.HipMem())


def test_gpu_jpeg_into_the_encoder(oracle, gpu_codec):
    JC.run_into_encoder(oracle, gpu_codec, MC.HipMem())


def test_gpu_jpeg_into_the_uastc_encoder(oracle):
    import uvol
    cu = uvol.Codec(device=0, uastc=1)
    try:
        JC.run_into_encoder(oracle, cu, MC.HipMem(), uastc=True)
    finally:
        cu.close()


def test_gpu_jpeg_bad_arguments_and_trim():
    import uvol
    cd = uvol.Codec(device=0)          # a context of its own: uvol_trim gives back workspaces the shared context's other tests hold
    try:
        mem = MC.HipMem()
        ptrs, want = JC.run_bad_arguments(cd, uvol.UvolError)
        assert np.array_equal(JC.read_layers(mem, ptrs, 16, 16)[0], want)
        cd.trim()
        P, want = JC.reference("c420_17x9")
        ptrs = cd.idct_jpeg_batch_dev([P.coef], [P.qt], P.w, P.h, 3, 2, 2, slot=1)
        assert np.array_equal(JC.read_layers(mem, ptrs, P.w, P.h)[0], want)
    finally:
        cd.close()


@pytest.mark.parametrize("name", sorted(JC.DRIVER_RUNS))
def test_gpu_uvolenc_jpeg_sequence(oracle, tmp_path, name):
    JC.run_driver(oracle, os.path.join(BIN, "uvolenc"), str(tmp_path), name)


def test_gpu_uvolenc_jpeg_corrupt_frame_fails_its_segment(oracle, tmp_path):
    JC.run_driver_corrupt_frame(oracle, os.path.join(BIN, "uvolenc"), str(tmp_path))


def test_gpu_basisu_shim_reads_jpeg(oracle, tmp_path):
    JC.run_basisu_shim(oracle, os.path.join(BIN, "basisu"), str(tmp_path))
