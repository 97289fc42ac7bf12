"""The calling conventions of the C ABI (tests/abi_surface_cases.py, shared with tests/test_hipemu_abi_surface.py) on a real MI355X."""
import pytest
import abi_surface_cases as AC
import material_cases as MC

pytestmark = pytest.mark.gpu


@pytest.fixture()
def make():
    import uvol
    return lambda **cfg: uvol.Codec(device=0, **cfg)


def test_gpu_abi_group_loop(make):
    AC.run_group_loop(make)


def test_gpu_abi_points_and_packed_fail_per_frame(make):
    AC.run_points_packed(make)


def test_gpu_abi_rejected_before_any_work(make):
    AC.run_rejected_before_work(make)


def test_gpu_abi_decode_and_transcode_entry_points(make):
    AC.run_decode_entries(make, MC.HipMem())


def test_gpu_abi_texture_encode_forms(make):
    AC.run_texture_encode_forms(make, MC.HipMem())


def test_gpu_abi_ragged_segments_are_refused(make):
    AC.run_ragged_segments_refused(make)


def test_gpu_abi_mesh_enqueue(make):
    AC.run_mesh_enqueue(make)


def test_gpu_abi_binding_intake(make):
    AC.run_binding_intake(make, MC.HipMem())
