"""Materials that meet at shared vertices (`material_seams = 1`) on the MI355X, through the C ABI and the hosts.  The checks are in
tests/material_seam_cases.py; tests/test_hipemu_material_seams.py runs them through the host emulation."""
import os
import subprocess
import sys
import numpy as np
import pytest
import material_cases as MC
import material_seam_cases as SC
from conftest import ROOT

pytestmark = pytest.mark.gpu
PKG = os.path.join(ROOT, "universal-volumetric_amd")


@pytest.fixture(scope="module")
def seam_codec():
    import uvol
    c = uvol.Codec(device=0, material_seams=1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def default_digest(oracle, seam_codec):
    return SC.forms_digest(oracle, seam_codec)


def test_gpu_material_seams_streams(oracle, seam_codec):
    """Checks 1 - 5 on every id pattern."""
    SC.run_streams(oracle, seam_codec, SC.seam_frames())


def test_gpu_material_seams_shuffled_storage(oracle, seam_codec):
    SC.run_streams(oracle, seam_codec, SC.shuffled(SC.seam_frames()))


def test_gpu_material_seams_frames_without_seams_keep_their_bytes(oracle, seam_codec, gpu_codec):
    """Check 6."""
    SC.run_unchanged_without_seams(oracle, seam_codec, gpu_codec)


def test_gpu_material_seams_default_still_refuses(oracle, seam_codec, gpu_codec):
    """Check 7."""
    SC.run_default_refuses(oracle, seam_codec, gpu_codec)


def test_gpu_material_seams_ragged_batch(oracle, seam_codec):
    """Check 8."""
    SC.run_ragged(oracle, seam_codec, MC.HipMem())


@pytest.mark.parametrize("force", ["relabel", "simt", "earlyjoin"])
def test_gpu_material_seams_kernel_forms(force, default_digest):
    """Check 9: fresh processes with the forms large calls take; the default forms' bytes; the 40 x 28 checkerboard took the retry."""
    code = ("import sys; sys.path[:0] = [%r, %r, %r]\n"
            "import uvol, oracle as O, material_seam_cases as SC\n"
            "O.lib(); cd = uvol.Codec(device=0, material_seams=1)\n"
            "print('digest', SC.forms_digest(O, cd))\n") % (os.path.join(ROOT, "tests"), PKG, os.path.join(ROOT, "oracle"))
    env = {"relabel": dict(UVOL_RELABEL="1"), "simt": dict(UVOL_SIMT_W="5", UVOL_ENTROPY_W="8"), "earlyjoin": dict(UVOL_LATE_JOIN="0")}[force]
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, UVOL_TIMING="1", **env), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "digest" in r.stdout, (r.stdout[-500:], r.stderr[-2500:])
    assert "re-encoding with worst-case workspace" in r.stderr
    assert r.stdout.split("digest")[1].split()[0] == default_digest


BIN = os.path.join(PKG, "bin")


def _two_material_obj(tmp_path, name="two.obj"):
    """The two-material OBJ of test_gpu_material_argv_shim: the small sphere, `usemtl body` on the first half of its faces, `usemtl prop`
    on the second.  -> (path, mesh, ids by first appearance of the name)."""
    import cli_helpers, synth
    m = synth.sphere_mesh(16, 9, charts=(2, 2))
    base = os.path.join(str(tmp_path), "plain_" + name); cli_helpers.write_obj(base, m, short=True)
    lines = open(base).read().splitlines(True)
    first_f = next(i for i, l in enumerate(lines) if l.startswith("f ")); nf = len(lines) - first_f
    assert nf == MC.nfaces(m)
    two = os.path.join(str(tmp_path), name)
    open(two, "w").write("".join(lines[:first_f] + ["usemtl body\n"] + lines[first_f:first_f + nf // 2] + ["usemtl prop\n"] + lines[first_f + nf // 2:]))
    fm = np.zeros(nf, np.uint8); fm[nf // 2:] = 1
    return two, m, fm


def _check_written(oracle, path, m, fm):
    """Four decoders, dec_type 1, the ids right by the matching."""
    d = oracle.drc_decode(open(path, "rb").read())
    assert d.leftover == 0 and len(d.atts) == 4 and d.atts[3]["dec_type"] == 1, (len(d.atts), d.atts[-1]["dec_type"])
    src = SC.match_faces(m, d)
    fv = MC.face_values(d)
    assert np.array_equal(fv[:, 0], fv[:, 1]) and np.array_equal(fv[:, 0], fv[:, 2]) and np.array_equal(fv[:, 0], fm[src])


def test_gpu_material_seams_argv_shim(oracle, tmp_path):
    """Check 11, the draco_encoder shim: with UVOL_MATERIAL_SEAMS=1 the seamed file is written with its materials and stderr has no line
    about them; without it, the fallback and its message remain."""
    subprocess.check_call(["make", "-s", "-C", PKG, "all"])
    two, m, fm = _two_material_obj(tmp_path)
    out = os.path.join(str(tmp_path), "two.drc")
    cmd = [os.path.join(BIN, "draco_encoder"), "-i", two, "-o", out, "-qp", "11", "-qt", "10", "-qn", "8", "-qg", "8", "-cl", "7"]
    r = subprocess.run(cmd, env=dict(os.environ, UVOL_MATERIAL_SEAMS="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "material" not in r.stderr, r.stderr
    _check_written(oracle, out, m, fm)
    env = {k: v for k, v in os.environ.items() if k != "UVOL_MATERIAL_SEAMS"}
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "material" in r.stderr and len(oracle.drc_decode(open(out, "rb").read()).atts) == 3


@pytest.mark.parametrize("how", ["env", "flag"])
def test_gpu_material_seams_uvolenc(oracle, tmp_path, how):
    """Check 11, the host driver: UVOL_MATERIAL_SEAMS=1 / --material-seams set the parameter; the seamed frame keeps its materials, no
    "material" line on stderr."""
    import cli_helpers
    subprocess.check_call(["make", "-s", "-C", PKG, "all"])
    cfgp, cfg, meshes, texs = cli_helpers.make_sequence(str(tmp_path), n_frames=3, tex=64, batch=3)
    fms = []
    for k in range(3):
        p = os.path.join(str(tmp_path), "OBJ", "frame_%05d.obj" % k); lines = open(p).read().splitlines(True)
        first_f = next(i for i, l in enumerate(lines) if l.startswith("f ")); nf = len(lines) - first_f
        fm = np.zeros(nf, np.uint8)
        if k == 1: fm[nf // 2:] = 1
        open(p, "w").write("".join(lines[:first_f] + ["usemtl body\n"] + (lines[first_f:] if k != 1 else lines[first_f:first_f + nf // 2] + ["usemtl prop\n"] + lines[first_f + nf // 2:])))
        fms.append(fm)
    env = {k: v for k, v in os.environ.items() if k != "UVOL_MATERIAL_SEAMS"}
    cmd = [os.path.join(BIN, "uvolenc"), cfgp] + (["--material-seams"] if how == "flag" else [])
    if how == "env": env["UVOL_MATERIAL_SEAMS"] = "1"
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert not [l for l in r.stderr.splitlines() if "material" in l], r.stderr
    pin = MC.stock_pin(oracle)
    for k, m in enumerate(meshes):
        path = os.path.join(cfg["OutputDirectory"], "geometry_draco", "%05d.drc" % k)
        if k == 1: _check_written(oracle, path, m, fms[k])
        else: MC.check_stock_row(oracle, open(path, "rb").read(), pin)
