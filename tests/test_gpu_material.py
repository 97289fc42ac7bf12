"""The OBJ material attribute (Draco GENERIC uint8, `usemtl`) on a real MI355X, through the C ABI: the checks of
tests/material_cases.py (shared with tests/test_hipemu_material.py), the argv shim, and one enqueued call at the bench's size."""
import os
import shlex
import subprocess
import sys
import numpy as np
import pytest
import material_cases as MC
from conftest import ROOT

pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "universal-volumetric_amd", "bin")


def test_gpu_material_stock_row_and_section(oracle, gpu_codec):
    """Check 1, also on the mesh the oracle decodes out of the recorded 00000.drc, re-encoded with material 0."""
    MC.run_stock_pin(oracle, gpu_codec, extra=[MC.reference_frame(oracle)])


def test_gpu_material_ragged_batch_and_null_entries(oracle, gpu_codec):
    MC.run_ragged_batch(oracle, gpu_codec)


def test_gpu_material_values_and_decoder(oracle, gpu_codec):
    """Checks 3 and 5: the ids come back through the oracle and through uvol_decode_mesh_batch_mat (host and device output form)."""
    streams = MC.run_values(oracle, gpu_codec)
    MC.run_decoder(oracle, gpu_codec, MC.HipMem(), streams)


@pytest.mark.parametrize("force", ["relabel", "simt"])
def test_gpu_material_shuffled_order_and_kernel_forms(force):
    """Check 3 with shuffled storage (relabelling forced on) and through the lane-per-walker kernels / lane-per-stream coder."""
    code = ("import sys; sys.path[:0] = [%r, %r, %r]\n"
            "import uvol, oracle as O, material_cases as MC\n"
            "O.lib(); cd = uvol.Codec(device=0)\n"
            "MC.run_shuffled(O, cd); MC.run_values(O, cd); MC.run_stock_pin(O, cd); cd.close(); print('ok')\n") % (
                os.path.join(ROOT, "tests"), os.path.join(ROOT, "universal-volumetric_amd"), os.path.join(ROOT, "oracle"))
    env = {"relabel": dict(UVOL_RELABEL="1"), "simt": dict(UVOL_SIMT_W="5", UVOL_ENTROPY_W="8")}[force]
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout[-500:], r.stderr[-2500:])


def test_gpu_material_interior_seam_is_refused_per_frame(oracle, gpu_codec):
    MC.run_refusal(oracle, gpu_codec)


def test_gpu_material_obj_ingest(oracle, gpu_codec, tmp_path):
    MC.run_ingest(oracle, gpu_codec, MC.HipMem(), tmp_path)


def test_gpu_material_argv_shim(oracle, tmp_path):
    """Check 7: the reference's exact argv on an OBJ with one usemtl line -> four decoders and the fixture's section; the same OBJ without
    the line -> today's bytes; a seamed two-material OBJ still produces a (three-decoder) file and stderr names it."""
    import cli_helpers, synth
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "universal-volumetric_amd"), "all"])
    pin = MC.stock_pin(oracle)
    m = synth.sphere_mesh(16, 9, charts=(2, 2))
    base = os.path.join(str(tmp_path), "plain.obj"); cli_helpers.write_obj(base, m, short=True)
    lines = open(base).read().splitlines(True)
    first_f = next(i for i, l in enumerate(lines) if l.startswith("f "))
    one = os.path.join(str(tmp_path), "one.obj"); open(one, "w").write("".join(lines[:first_f] + ["usemtl body\n"] + lines[first_f:]))
    nf = len(lines) - first_f
    two = os.path.join(str(tmp_path), "two.obj"); open(two, "w").write("".join(lines[:first_f] + ["usemtl body\n"] + lines[first_f:first_f + nf // 2] + ["usemtl prop\n"] + lines[first_f + nf // 2:]))
    out = {}
    for name, obj in (("plain", base), ("one", one), ("two", two)):
        drc = os.path.join(str(tmp_path), name + ".drc")
        cmd = f'{os.path.join(BIN, "draco_encoder")} -i "{obj}" -o "{drc}" -qp 11 -qt 10 -qn 8 -qg 8 -cl 7'
        r = subprocess.run(shlex.split(cmd), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        out[name] = (open(drc, "rb").read(), r.stderr)
    want = oracle.drc_encode(m["pos"], m["idx_pos"], m["uv"], m["idx_uv"], m["nrm"], m["idx_nrm"])
    # (write_obj prints 9 significant digits: the parsed floats are the mesh's own)
    assert out["plain"][0] == want
    d, a = MC.check_stock_row(oracle, out["one"][0], pin)
    assert out["one"][0][a["sec_begin"]:a["sec_end"]] == pin[1]
    MC.check_against_plain(oracle, out["one"][0], out["plain"][0])
    assert out["two"][0] == want and "two.obj" in out["two"][1] and "material" in out["two"][1]
    assert "material" not in out["one"][1] and "material" not in out["plain"][1]
    # at DRACO_COMPRESSION_LEVEL 0 the attribute is left out, with a line on stderr
    drc0 = os.path.join(str(tmp_path), "cl0.drc")
    r = subprocess.run([os.path.join(BIN, "draco_encoder"), "-i", one, "-o", drc0, "-cl", "0"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "one.obj" in r.stderr and "material" in r.stderr
    assert open(drc0, "rb").read() == oracle.drc_encode(m["pos"], m["idx_pos"], m["uv"], m["idx_uv"], m["nrm"], m["idx_nrm"], method=2)


def test_gpu_material_uvolenc_passes_ids_and_falls_back(oracle, tmp_path):
    """The host driver: device-parsed and host-parsed OBJ files with a usemtl line get the attribute; a seamed file is written without it."""
    import cli_helpers
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "universal-volumetric_amd"), "all"])
    cfgp, cfg, meshes, texs = cli_helpers.make_sequence(str(tmp_path), n_frames=6, tex=64, batch=3)
    for k in range(6):
        p = os.path.join(str(tmp_path), "OBJ", "frame_%05d.obj" % k); lines = open(p).read().splitlines(True)
        first_f = next(i for i, l in enumerate(lines) if l.startswith("f ")); nf = len(lines) - first_f
        if k == 5: continue                                                     # one file without materials
        ins = lines[:first_f] + ["usemtl body\n"] + (lines[first_f:] if k != 4 else lines[first_f:first_f + nf // 2] + ["usemtl prop\n"] + lines[first_f + nf // 2:])
        open(p, "w").write("".join(ins))
    r = subprocess.run([os.path.join(BIN, "uvolenc"), cfgp], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    pin = MC.stock_pin(oracle)
    for k, m in enumerate(meshes):
        got = open(os.path.join(cfg["OutputDirectory"], "geometry_draco", "%05d.drc" % k), "rb").read()
        want = oracle.drc_encode(m["pos"], m["idx_pos"], m["uv"], m["idx_uv"], m["nrm"], m["idx_nrm"])
        if k >= 4:
            assert got == want, k
        else:
            d, a = MC.check_stock_row(oracle, got, pin); assert got[a["sec_begin"]:a["sec_end"]] == pin[1]
            MC.check_against_plain(oracle, got, want)
    noted = [l for l in r.stderr.splitlines() if "material" in l]
    assert len(noted) == 1 and "frame_00004.obj" in noted[0]


def test_gpu_material_at_bench_size():
    """Check 8: ONE enqueued _mat call of 800 frames of the bench's mesh generator (100 k vertices, 400 distinct connectivities, each
    stored twice), material 0 on every frame.  A call of this size takes the lane-per-walker kernels (more walkers than the LDS forms
    hold: > 3 per CU) and the lane-per-stream coder - another code path than the small meshes of the other checks.  A seeded sample is
    checked against the fixture's row / section and against the material-less stream; all equal-content pairs are equal."""
    import synth, uvol, oracle as O
    O.lib()
    nd, n = 400, 800
    distinct = synth.distinct_meshes(nd, bases=16)
    zeros = np.zeros(max(MC.nfaces(f) for f in distinct), np.uint8)
    frames = [dict(distinct[i % nd], face_mat=zeros[:MC.nfaces(distinct[i % nd])]) for i in range(n)]
    cd = uvol.Codec(device=0, max_batch=n)
    try:
        cd.start_mesh_batch(frames)
        res = cd.finish()[0]
        sample = sorted(int(i) for i in np.random.default_rng(8).choice(n, 10, replace=False))
        base = cd.encode_mesh_batch([MC.plain(frames[i]) for i in sample])
    finally:
        cd.close()
    assert len(res) == n and all(r is not None for r in res)
    pin = MC.stock_pin(O)
    for i, b in zip(sample, base):
        d, a = MC.check_stock_row(O, res[i], pin)
        assert res[i][a["sec_begin"]:a["sec_end"]] == pin[1], i
        MC.check_against_plain(O, res[i], b)
    for i in range(nd):
        assert res[i] == res[i + nd], i
