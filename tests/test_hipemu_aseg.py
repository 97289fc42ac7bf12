"""Attribute vertices from the face seam flags (k_aseg: one thread per face, one walk per fan segment; the id-space sizes from
k_pack_tabs), through the host emulation of the kernels (tests/hipemu, no GPU).  The batch
and what each of its frames is there for: tests/aseg_cases.py.  The emulation runs a kernel's threads one after the other, so it checks
the rule - which corners are written, with what - and not the order in which the segments draw their ids, which only the GPU varies
(tests/test_gpu_aseg.py)."""
import os
import subprocess
import sys
import pytest
from conftest import ROOT
import aseg_cases as AC
from aseg_cases import FORMS, RETRY


def test_aseg_cases_are_what_they_say():
    """The hand-built frames hold the seams their descriptions name (counted from the index arrays alone)."""
    fs = AC.frames()
    assert AC.seam_census(fs[0], "uv")[2] == 1 and AC.seam_census(fs[0], "nrm")[1] == 0            # one dead end inside; the other end is on the border
    assert AC.seam_census(fs[1], "nrm")[2] == 2 and AC.seam_census(fs[1], "uv")[1] == 0            # both ends inside
    assert AC.seam_census(fs[2], "uv")[1] == 3 and AC.seam_census(fs[2], "nrm")[1] == 4            # three and four seams meet
    assert AC.seam_census(fs[3], "uv")[0] == 1 and AC.seam_census(fs[3], "nrm")[2] == 1            # a chart of one face
    assert AC.seam_census(fs[5], "uv") == (0, 0, 0) and AC.seam_census(fs[5], "nrm") == (0, 0, 0)
    assert AC.seam_census(fs[6], "uv")[1] == 0 and AC.seam_census(fs[6], "nrm")[1] == 0
    assert "uv" not in fs[4] and len(fs) == AC.N_FRAMES
    assert all(len(f["idx_pos"]) // 3 == 330 for f in fs[:5])          # more than one block of 256 faces, the last one partly filled
    o = AC.overflow_frame(); nv = len(o["pos"])
    assert 3 * AC.seam_census(o, "uv")[0] > nv // 2 + 4096            # every corner of a one-face chart is a segment: more of them than ecap - V ids


@pytest.mark.parametrize("form", sorted(FORMS))
def test_hipemu_aseg_batch_of_13(hipemu_lib, form):
    """Every frame of the batch equals oracle.drc_encode byte for byte, with the LDS walkers and with per-face records; the frame whose
    segments exceed the entry capacity fails on the device with the workspace-overflow status - the host then says that it encodes it
    again, once - and comes out right, as do its neighbours.  The switches are read once per process, hence the fresh interpreter."""
    code = ("import sys; sys.path[:0] = [%r, %r, %r]\n"
            "import uvol, oracle as O, aseg_cases as AC\n"
            "O.lib(); cd = uvol.Codec(lib_path=%r)\n"
            "AC.run_batch(O, cd); cd.close(); print('ok')\n") % (
                os.path.join(ROOT, "tests"), os.path.join(ROOT, "universal-volumetric_amd"), os.path.join(ROOT, "oracle"), hipemu_lib)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, UVOL_TIMING="1", **FORMS[form]), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout[-500:], r.stderr[-2500:])
    assert r.stderr.count(RETRY) == 1 and "mesh 1: " + RETRY in r.stderr, r.stderr[-2500:]
