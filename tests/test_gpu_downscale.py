"""The device downscale (uvol_downscale_rgba_batch_dev, csrc/tex_downscale.hip) on a real MI355X, through the C ABI, and `uvolenc
--texture-ladder` with the real binaries: the checks of tests/downscale_cases.py (shared with tests/test_hipemu_downscale.py)."""
import os
import pytest
import downscale_cases as DC
import material_cases as MC
from conftest import ROOT

pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "universal-volumetric_amd", "bin")


def test_gpu_downscale_bit_exact_shapes(gpu_codec):
    DC.run_shapes(gpu_codec, MC.HipMem())


def test_gpu_downscale_layers_of_an_ingest_slot(gpu_codec):
    from test_hipemu_tex import png_scanlines
    DC.run_ingest_slot(gpu_codec, MC.HipMem(), png_scanlines)


def test_gpu_downscale_host_inputs(gpu_codec):
    DC.run_host_inputs(gpu_codec, MC.HipMem())


def test_gpu_downscale_arithmetic_edges(gpu_codec):
    DC.run_arithmetic_edges(gpu_codec, MC.HipMem())


def test_gpu_downscale_into_the_encoder(oracle, gpu_codec):
    DC.run_into_encoder(oracle, gpu_codec, MC.HipMem())


def test_gpu_downscale_into_the_uastc_encoder(oracle):
    import uvol
    cu = uvol.Codec(device=0, uastc=1)
    try:
        DC.run_into_encoder(oracle, cu, MC.HipMem(), uastc=True)
    finally:
        cu.close()


def test_gpu_downscale_slots_trim_and_refusals():
    import uvol
    cd = uvol.Codec(device=0)          # a context of its own: uvol_trim gives back workspaces the shared context's other tests hold
    try:
        DC.run_slots(cd, MC.HipMem())
        DC.run_refusals(cd, MC.HipMem(), uvol.UvolError)
    finally:
        cd.close()


def test_gpu_uvolenc_texture_ladder(oracle, gpu_codec, tmp_path):
    DC.run_driver(oracle, os.path.join(BIN, "uvolenc"), str(tmp_path), gpu_codec.ktx2_info)
