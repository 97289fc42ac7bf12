"""The packed render-ready mesh decode (uvol_decode_mesh_batch_packed) on a real MI355X, through the C ABI: the checks of
tests/packed_cases.py (shared with tests/test_hipemu_packed.py), with all 250 recorded files."""
import pytest
import material_cases as MC
import packed_cases as KC
import points_cases as PC

pytestmark = pytest.mark.gpu


@pytest.fixture()
def gpu_codec0():
    import uvol
    c = uvol.Codec(device=0, DRACO_COMPRESSION_LEVEL=0)
    yield c
    c.close()


def test_gpu_packed_all_recorded_files(oracle):
    """Checks 1 and 2: all 250 recorded files in batches of 50: records, index, counts, flags and transform against the reference; index and
    n_points against uvol_decode_mesh_batch_points."""
    import uvol
    cd = uvol.Codec(device=0, max_batch=50)
    try:
        assert KC.run_recorded(oracle, cd, PC.recorded_files(), batch=50) == 250
    finally:
        cd.close()


def test_gpu_packed_attribute_subsets_and_tool_sets(oracle, gpu_codec, gpu_codec0):
    KC.run_subsets(oracle, gpu_codec, gpu_codec0)


def test_gpu_packed_materials(oracle, gpu_codec):
    KC.run_materials(oracle, gpu_codec)


def test_gpu_packed_ragged_batch_fails_per_frame(oracle, gpu_codec, gpu_codec0):
    KC.run_ragged(oracle, gpu_codec, gpu_codec0, MC.HipMem())


def test_gpu_packed_more_than_16_bits_is_refused_alone(oracle, gpu_codec):
    KC.run_wide_quantisation(oracle, gpu_codec)


def test_gpu_packed_memory_forms(oracle, gpu_codec, gpu_codec0):
    """Check 7: records in HBM (written in place by k_weld_write_packed), in pageable host memory and in a PinnedArena."""
    KC.run_memory_forms(oracle, gpu_codec, gpu_codec0, MC.HipMem(), extra=KC.golden("00075.drc"))


def test_gpu_packed_existing_entry_points_untouched(oracle, gpu_codec, gpu_codec0):
    files = [f for _, f in PC.subset_streams(gpu_codec, gpu_codec0)][:5] + [KC.run_materials_stream(gpu_codec)] + KC.golden("00000.drc", "00075.drc")
    KC.run_existing_untouched(oracle, gpu_codec, files)
