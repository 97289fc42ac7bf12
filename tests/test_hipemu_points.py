"""The render-ready mesh decode (uvol_decode_mesh_batch_points) through the host emulation of the kernels (tests/hipemu, no GPU): decode
kernels -> weld kernels (csrc/geo_weld.hpp) -> one index per corner + one value record per point, against a NumPy reference built from the
oracle decoder's output.  The checks are in tests/points_cases.py; tests/test_gpu_points.py runs the same ones on the MI355X."""
import os
import pytest
import material_cases as MC
import points_cases as PC
from conftest import GOLDEN


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


def test_hipemu_points_recorded_files(oracle, emu):
    """Check 1: 26 of the 250 recorded files (every 10th - 00000 is one of them - and 00075), both layouts, bit-exact against the reference;
    the renderer's invariant against the existing decode on 00000 and 00075 only.  The trade-off: the invariant needs a third decode of
    every file it covers (uvol_decode_mesh_batch beside the two layouts), and the emulation runs the decoder's one-lane stages at several
    seconds per recorded frame - this test already takes about 8 minutes of wall time on 16 cores (measured: 489 s), well past the
    minute one would like for it, and 24 more decodes would add about a third.  The reference check, which is the stronger one (it
    fixes numbering and values, the invariant follows from it and the existing decode's own oracle test), runs on all 26;
    tests/test_gpu_points.py asserts the invariant on all 250."""
    files = PC.recorded_files(step=10)
    two = [i for i, f in enumerate(files) if f in [open(os.path.join(GOLDEN, n), "rb").read() for n in ("00000.drc", "00075.drc")]]
    assert len(two) == 2 and PC.run_recorded(oracle, emu, files, invariant_on=two) == 26


def test_hipemu_points_attribute_subsets_and_tool_sets(oracle, emu, emu0):
    """Check 2: positions only, positions + uv, positions + normals, all three with seams, a polygon soup, two `-cl 0` streams."""
    PC.run_subsets(oracle, emu, emu0)


def test_hipemu_points_ragged_batch_fails_per_frame(oracle, emu, emu0):
    """Check 3: a truncated file, a foreign file, a frame one point short and a frame one face short fail alone."""
    PC.run_ragged(oracle, emu, emu0)


def test_hipemu_points_long_fan_is_refused_alone(oracle, emu, emu0):
    """The weld's documented limit: more than 4096 corners on one position entry -> UVOL_E_UNSUPPORTED for that frame alone."""
    PC.run_long_fan(oracle, emu, emu0)


def test_hipemu_points_memory_forms(oracle, emu, emu0, hipemu_lib):
    """Check 4: "device" outputs (the emulation's device memory is host memory), pageable host outputs, outputs in a PinnedArena."""
    PC.run_memory_forms(oracle, emu, emu0, MC.HostMem(), lib_path=hipemu_lib)


def test_hipemu_points_round_trip_through_the_encoder(oracle, emu):
    """Check 5: welded buffers -> encoder (host form, one index stream) -> oracle decoder: same faces, positions within one quantiser step."""
    PC.run_round_trip(oracle, emu)


def test_hipemu_points_existing_decode_untouched(oracle, emu, emu0):
    """Check 6: uvol_decode_mesh_batch[_mat] on the same files is the oracle's decode and records no kernel group of the weld."""
    files = [f for _, f in PC.subset_streams(emu, emu0)][:5] + [open(os.path.join(GOLDEN, "00000.drc"), "rb").read()]
    PC.run_existing_untouched(oracle, emu, files)
