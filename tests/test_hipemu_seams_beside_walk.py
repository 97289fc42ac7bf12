"""The two forms of the group enqueue - the valence replay on the lane's auxiliary stream joined behind the traversals (late, now also at
bench scale where device memory allows) or before the record tables (early) - through the host emulation of the kernels (tests/hipemu,
no GPU).  The emulation
runs the streams one after the other in the order of the enqueue: it checks the data flow - what each kernel reads has been written, and
no array a later kernel still reads lies where another was placed - not the concurrency.  In particular a lifetime of the replay's
inputs that ended too early for the late join would NOT show here: the replay has run to its end before the traversals start.  That
shows only on the GPU (tests/test_gpu_seams_beside_walk.py, on small frames in the LDS-walker layout; the bench-scale layout - compact,
per-face records - runs late-joined in tests/test_gpu_geom.py's 1280-frame call when memory allows, and in bench.py --full's parity)."""
import os
import subprocess
import sys
import pytest
from conftest import ROOT

FORMS = {"early": dict(UVOL_LATE_JOIN="0"), "late": dict(UVOL_LATE_JOIN="1"),
         "early_simt": dict(UVOL_LATE_JOIN="0", UVOL_SIMT_W="5", UVOL_ENTROPY_W="8"), "late_simt": dict(UVOL_LATE_JOIN="1", UVOL_SIMT_W="5", UVOL_ENTROPY_W="8")}


@pytest.mark.parametrize("form", sorted(FORMS))
def test_hipemu_seams_beside_walk_batch_of_19(hipemu_lib, form):
    """19 distinct frames (seamed spheres, tori, a positions-only frame, open meshes, one refused frame) with the join forced early and
    late, each with the LDS walkers and with the lane-per-walker kernels / lane-per-stream coder (5 walkers and 8 streams per wave: 19 is
    no multiple of either).  Every good frame equals oracle.drc_encode byte for byte, the refused frame keeps its status.  The switches
    are read once per process, hence the fresh interpreter."""
    code = ("import sys; sys.path[:0] = [%r, %r, %r]\n"
            "import uvol, oracle as O, seams_beside_walk_cases as SC\n"
            "O.lib(); cd = uvol.Codec(lib_path=%r)\n"
            "SC.run_batch(O, cd); cd.close(); print('ok')\n") % (
                os.path.join(ROOT, "tests"), os.path.join(ROOT, "universal-volumetric_amd"), os.path.join(ROOT, "oracle"), hipemu_lib)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **FORMS[form]), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout[-500:], r.stderr[-2500:])


def test_hipemu_seams_beside_walk_workspace_is_unchanged(hipemu_lib):
    """uvol_mesh_workspace of four distinct 100 k-vertex frames and one sphere, default parameters: the values of the commit before the
    late join moved behind the traversals (recorded with its emulation build).  The entry point lays a frame out with the EARLY join
    and takes the larger of the large-batch and the small-call form, so this pins the early layout and the arrays' sizes only: it would
    not notice another place of the late join, and it is not what a frame of a late-joined large call holds (about 5 MB more for these
    meshes)."""
    import synth, uvol
    cd = uvol.Codec(lib_path=hipemu_lib)
    try:
        meshes = synth.distinct_meshes(4, 400, 251) + [synth.sphere_mesh(400, 251, frame=0, seed=0)]
        assert [cd.mesh_workspace(**m) for m in meshes] == [49339752, 49333240, 49342136, 49825192, 49363816]
    finally:
        cd.close()
