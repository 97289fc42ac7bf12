"""Decoding the corner-form material attribute (files written with `material_seams = 1`) on a real MI355X, through the C ABI: checks 1 - 5 of
tests/material_seam_decode_cases.py (shared with tests/test_hipemu_material_seam_decode.py, which also holds the corrupt-file check)."""
import pytest
import material_cases as MC
import material_seam_cases as SC
import material_seam_decode_cases as DC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu_seams():
    import uvol
    cd = uvol.Codec(device=0, material_seams=1)
    yield cd
    cd.close()


@pytest.fixture(scope="module")
def seam_files(gpu_seams):
    frs = DC.frames()
    return [f[0] for f in frs], DC.encode(gpu_seams, frs)


def test_gpu_seam_decode_mat_every_frame(oracle, gpu_seams, seam_files):
    """Check 1: has_mat, face_mat and the six arrays on every frame, host and device outputs."""
    DC.run_mat(oracle, gpu_seams, MC.HipMem(), seam_files[1], slots=[2] * len(seam_files[1]))


def test_gpu_seam_decode_mat_shuffled_storage(oracle, gpu_seams):
    DC.run_mat(oracle, gpu_seams, MC.HipMem(), DC.encode(gpu_seams, SC.shuffled(DC.frames())))


def test_gpu_seam_decode_workspace_retry(oracle, gpu_seams):
    DC.run_retry(oracle, gpu_seams)


def test_gpu_seam_decode_three_slots(oracle, gpu_seams):
    """Check 2: the material in attribute-data slot 2, 1 and 0."""
    DC.run_mat(oracle, gpu_seams, MC.HipMem(), DC.slot_files(gpu_seams), slots=[2, 1, 0])


def test_gpu_seam_decode_packed(oracle, gpu_seams, seam_files):
    """Check 3 on the files of checks 1 and 2."""
    DC.run_packed(oracle, gpu_seams, seam_files[1], seam_files[0])
    DC.run_packed(oracle, gpu_seams, DC.slot_files(gpu_seams), ["slot2", "slot1", "slot0"])


def test_gpu_seam_decode_packed_point_counts(oracle, gpu_seams):
    DC.run_packed_point_counts(oracle, gpu_seams)


def test_gpu_seam_decode_ragged_batch(oracle, gpu_seams):
    """Check 4."""
    DC.run_ragged(oracle, gpu_seams)


def test_gpu_seam_decode_plain_calls_stay_plain(oracle, gpu_seams):
    """Check 5."""
    DC.run_plain_stays_plain(oracle, gpu_seams)
