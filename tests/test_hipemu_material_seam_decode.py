"""Decoding the corner-form material attribute (files written with `material_seams = 1`) through the host emulation of the kernels
(tests/hipemu, no GPU): uvol_decode_mesh_batch_mat and _packed read the material from the seam-cut table of its own attribute-data slot -
the third table through the pass of csrc/geo_mattab_dec.hpp -, the plain entry points skip it.  The checks are in
tests/material_seam_decode_cases.py; tests/test_gpu_material_seam_decode.py runs checks 1 - 5 on the MI355X."""
import pytest
import material_cases as MC
import material_seam_cases as SC
import material_seam_decode_cases as DC


@pytest.fixture(scope="module")
def emu(hipemu_lib):
    import uvol
    cd = uvol.Codec(lib_path=hipemu_lib, material_seams=1)
    yield cd
    cd.close()


@pytest.fixture(scope="module")
def seam_files(emu):
    frs = DC.frames()
    return [f[0] for f in frs], DC.encode(emu, frs)


def test_hipemu_seam_decode_mat_every_frame(oracle, emu, seam_files):
    """Check 1: has_mat, face_mat and the six arrays on every frame, host and device outputs."""
    DC.run_mat(oracle, emu, MC.HostMem(), seam_files[1], slots=[2] * len(seam_files[1]))


def test_hipemu_seam_decode_mat_shuffled_storage(oracle, emu):
    """Check 1 on the same frames with their faces stored in a seeded random order."""
    DC.run_mat(oracle, emu, MC.HostMem(), DC.encode(emu, SC.shuffled(DC.frames())))


def test_hipemu_seam_decode_workspace_retry(oracle, emu):
    DC.run_retry(oracle, emu)


def test_hipemu_seam_decode_three_slots(oracle, emu):
    """Check 2: the material in attribute-data slot 2, 1 and 0."""
    DC.run_mat(oracle, emu, MC.HostMem(), DC.slot_files(emu), slots=[2, 1, 0])


def test_hipemu_seam_decode_packed(oracle, emu, seam_files):
    """Check 3 on the files of checks 1 and 2."""
    DC.run_packed(oracle, emu, seam_files[1], seam_files[0])
    DC.run_packed(oracle, emu, DC.slot_files(emu), ["slot2", "slot1", "slot0"])


def test_hipemu_seam_decode_packed_point_counts(oracle, emu):
    DC.run_packed_point_counts(oracle, emu)


def test_hipemu_seam_decode_ragged_batch(oracle, emu):
    """Check 4."""
    DC.run_ragged(oracle, emu)


def test_hipemu_seam_decode_plain_calls_stay_plain(oracle, emu):
    """Check 5."""
    DC.run_plain_stays_plain(oracle, emu)


def test_hipemu_seam_decode_corrupt_files(oracle, emu):
    """Check 6 (no GPU counterpart)."""
    assert DC.run_corrupt(oracle, emu) > 40
