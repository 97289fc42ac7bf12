"""Attribute vertices from the face seam flags (k_aseg; the id-space sizes from k_pack_tabs) on the MI355X, where the segments of a
frame really draw their ids concurrently and in any order
(tests/test_hipemu_aseg.py checks the rule without a GPU).  The batch: tests/aseg_cases.py."""
import os
import subprocess
import sys
import pytest
from conftest import ROOT
from aseg_cases import FORMS, RETRY

pytestmark = pytest.mark.gpu

CODE = ("import sys; sys.path[:0] = [%r, %r, %r]\n"
        "import uvol, oracle as O, aseg_cases as AC\n"
        "O.lib(); cd = uvol.Codec(device=0)\n"
        "AC.run_batch(O, cd); cd.close(); print('ok')\n")


@pytest.mark.parametrize("form", sorted(FORMS))
def test_gpu_aseg_batch_of_13(form):
    """The 13 frames of aseg_cases in one call, then the frame whose segments exceed the entry capacity between two good ones: every
    frame byte-equal to the oracle, with the LDS walkers (the default of a small call) and with the lane-per-walker kernels on per-face
    records (the form of the large calls); the overflowing frame - and only it - is encoded a second time.  The switches are read once
    per process, hence the fresh interpreter."""
    code = CODE % (os.path.join(ROOT, "tests"), os.path.join(ROOT, "universal-volumetric_amd"), os.path.join(ROOT, "oracle"))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, UVOL_TIMING="1", **FORMS[form]), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout[-500:], r.stderr[-2500:])
    assert r.stderr.count(RETRY) == 1 and "mesh 1: " + RETRY in r.stderr, r.stderr[-2500:]
