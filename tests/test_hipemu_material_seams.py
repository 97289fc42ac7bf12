"""Materials that meet at shared vertices (`material_seams = 1`: the material attribute as a Draco corner attribute) through the host
emulation of the kernels (tests/hipemu, no GPU).  The checks are in tests/material_seam_cases.py; tests/test_gpu_material_seams.py runs
them on the MI355X."""
import os
import subprocess
import sys
import pytest
import material_cases as MC
import material_seam_cases as SC
from conftest import ROOT


@pytest.fixture(scope="module")
def emu_pair(hipemu_lib):
    import uvol
    cs, cd = uvol.Codec(lib_path=hipemu_lib, material_seams=1), uvol.Codec(lib_path=hipemu_lib)
    yield cs, cd
    cs.close(); cd.close()


def test_hipemu_material_seams_streams(oracle, emu_pair):
    """Checks 1 - 5 on every id pattern: row, everything else unchanged, seam stream, counts, values and the bound."""
    SC.run_streams(oracle, emu_pair[0], SC.seam_frames())


def test_hipemu_material_seams_shuffled_storage(oracle, emu_pair):
    """The same frames with their faces stored in a seeded random order."""
    SC.run_streams(oracle, emu_pair[0], SC.shuffled(SC.seam_frames()))


def test_hipemu_material_seams_frames_without_seams_keep_their_bytes(oracle, emu_pair):
    """Check 6: with the parameter set, frames with zeros, ids that follow connected components and no ids give the default codec's bytes."""
    SC.run_unchanged_without_seams(oracle, *emu_pair)


def test_hipemu_material_seams_default_still_refuses(oracle, emu_pair):
    """Check 7: the default codec refuses the frame the other one writes."""
    SC.run_default_refuses(oracle, *emu_pair)


def test_hipemu_material_seams_ragged_batch(oracle, emu_pair):
    """Check 8: a ragged batch; bytes do not depend on the batch, on where the inputs live, or on the form of the call."""
    SC.run_ragged(oracle, emu_pair[0], MC.HostMem())


@pytest.fixture(scope="module")
def default_digest(oracle, emu_pair):
    return SC.forms_digest(oracle, emu_pair[0])


@pytest.mark.parametrize("force", ["relabel", "simt", "earlyjoin"])
def test_hipemu_material_seams_kernel_forms(hipemu_lib, force, default_digest):
    """Check 9: the forms large calls take, forced by environment in a fresh process, give the bytes of the default forms.  The process
    that runs the default forms of the lot also reports its one-frame retries: the 40 x 28 checkerboard must have taken one."""
    code = ("import sys; sys.path[:0] = [%r, %r, %r]\n"
            "import uvol, oracle as O, material_seam_cases as SC\n"
            "O.lib(); cd = uvol.Codec(lib_path=%r, material_seams=1)\n"
            "print('digest', SC.forms_digest(O, cd))\n") % (
                os.path.join(ROOT, "tests"), os.path.join(ROOT, "universal-volumetric_amd"), os.path.join(ROOT, "oracle"), hipemu_lib)
    env = {"relabel": dict(UVOL_RELABEL="1"), "simt": dict(UVOL_SIMT_W="5", UVOL_ENTROPY_W="8"), "earlyjoin": dict(UVOL_LATE_JOIN="0")}[force]
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, UVOL_TIMING="1", **env), capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0 and "digest" in r.stdout, (r.stdout[-500:], r.stderr[-2500:])
    assert "re-encoding with worst-case workspace" in r.stderr
    assert r.stdout.split("digest")[1].split()[0] == default_digest
