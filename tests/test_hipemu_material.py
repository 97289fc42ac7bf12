"""The OBJ material attribute (Draco GENERIC uint8, `usemtl`) through the host emulation of the kernels (tests/hipemu, no GPU):
encode kernels -> .drc -> decode kernels, the C ABI's _mat entry points, the device OBJ parser and the host parser.  The checks are in
tests/material_cases.py; tests/test_gpu_material.py runs the same ones on the MI355X."""
import os
import subprocess
import sys
import pytest
import material_cases as MC
from conftest import ROOT


@pytest.fixture()
def emu(hipemu_lib):
    import uvol
    cd = uvol.Codec(lib_path=hipemu_lib)
    yield cd
    cd.close()


def test_hipemu_material_stock_row_and_section(oracle, emu):
    """Check 1: material 0 on every face gives the fourth decoder of the reference's recorded files - row and 18 section bytes."""
    MC.run_stock_pin(oracle, emu)


def test_hipemu_material_ragged_batch_and_null_entries(oracle, emu):
    """Check 2: frames without ids, NULL entries and a NULL array are the existing call, byte for byte; att_data_id follows nad."""
    MC.run_ragged_batch(oracle, emu)


def test_hipemu_material_values_come_back(oracle, emu):
    """Check 3: ids that follow connected shells are decoded on the faces they were given to; dropped faces take theirs with them."""
    MC.run_values(oracle, emu)


@pytest.mark.parametrize("force", ["relabel", "relabel_simt", "simt", "earlyjoin"])
def test_hipemu_material_shuffled_order_and_kernel_forms(hipemu_lib, force):
    """Check 3 with the faces stored in random order and the locality relabelling forced on (the ids are permuted with the faces), and
    the value frames through the lane-per-walker kernels / lane-per-stream coder and the early join.  The switches are read once per
    process, hence the fresh interpreter."""
    code = ("import sys; sys.path[:0] = [%r, %r, %r]\n"
            "import uvol, oracle as O, material_cases as MC\n"
            "O.lib(); cd = uvol.Codec(lib_path=%r)\n"
            "MC.run_shuffled(O, cd); MC.run_values(O, cd); MC.run_stock_pin(O, cd); print('ok')\n") % (
                os.path.join(ROOT, "tests"), os.path.join(ROOT, "universal-volumetric_amd"), os.path.join(ROOT, "oracle"), hipemu_lib)
    env = {"relabel": dict(UVOL_RELABEL="1"), "relabel_simt": dict(UVOL_RELABEL="1", UVOL_SIMT_W="7", UVOL_ENTROPY_W="8"),
           "simt": dict(UVOL_SIMT_W="5", UVOL_ENTROPY_W="8"), "earlyjoin": dict(UVOL_LATE_JOIN="0")}[force]
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout[-500:], r.stderr[-2500:])


def test_hipemu_material_interior_seam_is_refused_per_frame(oracle, emu, hipemu_lib):
    """Check 4: two ids meeting at shared vertices -> that frame UVOL_E_UNSUPPORTED, the batch's other frames unaffected; level 0 refuses the call."""
    MC.run_refusal(oracle, emu, lib_path=hipemu_lib)


def test_hipemu_material_decoder_hands_the_ids_back(oracle, emu):
    """Check 5: uvol_decode_mesh_batch_mat on the recorded files, on the streams of check 3 and on a three-decoder stream."""
    streams = MC.run_values(oracle, emu)
    MC.run_decoder(oracle, emu, MC.HostMem(), streams)


def test_hipemu_material_obj_ingest(oracle, emu, tmp_path):
    """Check 6: `usemtl` through read_obj and through the device parser: identical, expected ids."""
    MC.run_ingest(oracle, emu, MC.HostMem(), tmp_path)


def test_hipemu_material_less_workspace_is_unchanged(emu):
    """uvol_mesh_workspace of a frame without materials returns what it returned before the material attribute existed: the values below
    were recorded with the emulation build of the commit before it (default parameters), for these five meshes.  The bound of a frame with
    ids only grows."""
    import ctypes as C
    import synth
    t = synth.torus_mesh()
    meshes = MC.small_meshes() + [dict(pos=t["pos"], idx_pos=t["idx_pos"]), synth.sphere_mesh(120, 61, charts=(12, 6), frame=3)]
    recorded = [3928168, 3925608, 3870456, 3880552, 4652648]
    for f, want in zip(meshes, recorded):
        m, keep = emu._mesh_host(**MC.plain(f))
        assert emu.L.uvol_mesh_workspace(emu.h, C.byref(m)) == want
        assert emu.L.uvol_mesh_bound_mat(C.byref(m)) > emu.L.uvol_mesh_bound(C.byref(m))
