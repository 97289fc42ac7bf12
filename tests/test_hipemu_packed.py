"""The packed render-ready mesh decode (uvol_decode_mesh_batch_packed) through the host emulation of the kernels (tests/hipemu, no GPU):
decode kernels -> weld kernels (csrc/geo_weld.hpp, k_weld_write_packed) -> one index per corner + one 16-byte integer record per point,
against a NumPy reference built from the oracle decoder's output.  The checks are in tests/packed_cases.py; tests/test_gpu_packed.py runs
the same ones on the MI355X, with all 250 recorded files.  The emulation runs the decoder's one-lane stages at several seconds per recorded
frame (see tests/test_hipemu_points.py), so only 00000.drc and 00075.drc are decoded here."""
import pytest
import material_cases as MC
import packed_cases as KC
import points_cases as PC


@pytest.fixture()
def emu(hipemu_lib):
    import uvol
    cd = uvol.Codec(lib_path=hipemu_lib)
    yield cd
    cd.close()


@pytest.fixture()
def emu0(hipemu_lib):
    import uvol
    cd = uvol.Codec(lib_path=hipemu_lib, DRACO_COMPRESSION_LEVEL=0)
    yield cd
    cd.close()


def test_packed_dequantisation_formula_is_two_roundings(oracle):
    """Check 1, CPU only (no kernels): on every recorded file, float32 minv + q * scale with the product rounded before the sum is the
    oracle's float, bit for bit - the formula include/uvol_codec.h documents; the fused form is NOT what the oracle computes (its build
    switches contraction off), and on these files the two do differ somewhere, so the distinction is not idle."""
    files = PC.recorded_files()
    for f in files:
        KC.check_dequant_formula(oracle, f)
    import numpy as np
    a = oracle.drc_decode(files[0]).att("position")
    q = a["vals"].astype(np.float64); s = np.float64(KC.scale_of(a)); mn = np.array(a["minv"][:3], np.float64)
    fused = (mn[None, :] + q * s).astype(np.float32)                          # one rounding (exact in float64: 11-bit q, 24-bit scale)
    assert not PC.same_bits(fused, a["float"])


def test_packed_wide_stream_is_read_back_by_the_oracle(oracle):
    """Check 6, CPU half: the oracle encoder refuses qp = 17, so the case is its qp = 16 stream with the quantisation-bits byte rewritten
    to 17, which the oracle decoder reads back (packed_cases.wide_stream asserts each step)."""
    KC.wide_stream(oracle)


def test_hipemu_packed_recorded_files(oracle, emu):
    """Checks 1 and 2 on 00000.drc and 00075.drc."""
    assert KC.run_recorded(oracle, emu, KC.golden("00000.drc", "00075.drc")) == 2


def test_hipemu_packed_attribute_subsets_and_tool_sets(oracle, emu, emu0):
    KC.run_subsets(oracle, emu, emu0)


def test_hipemu_packed_materials(oracle, emu):
    KC.run_materials(oracle, emu)


def test_hipemu_packed_ragged_batch_fails_per_frame(oracle, emu, emu0):
    KC.run_ragged(oracle, emu, emu0, MC.HostMem())


def test_hipemu_packed_more_than_16_bits_is_refused_alone(oracle, emu):
    KC.run_wide_quantisation(oracle, emu)


def test_hipemu_packed_memory_forms(oracle, emu, emu0, hipemu_lib):
    KC.run_memory_forms(oracle, emu, emu0, MC.HostMem(), lib_path=hipemu_lib)


def test_hipemu_packed_existing_entry_points_untouched(oracle, emu, emu0):
    files = [f for _, f in PC.subset_streams(emu, emu0)][:5] + [KC.run_materials_stream(emu)]
    KC.run_existing_untouched(oracle, emu, files)
