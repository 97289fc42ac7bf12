"""End-to-end on a real GPU: `uvolenc project-config.json` (the Encoder.py-equivalent host driver) and the two argv shims."""
import json
import os
import shlex
import subprocess
import pytest
from conftest import ROOT

pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "universal-volumetric_amd", "bin")


def test_uvolenc_end_to_end(oracle, tmp_path):
    import cli_helpers
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "universal-volumetric_amd"), "all"])
    cfgp, cfg, meshes, texs = cli_helpers.make_sequence(str(tmp_path), n_frames=12, tex=64, batch=5)
    r = subprocess.run([os.path.join(BIN, "uvolenc"), cfgp, "--encoder-py-manifest"], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    out = cfg["OutputDirectory"]
    drc = sorted(os.listdir(os.path.join(out, "geometry_draco"))); ktx = sorted(os.listdir(os.path.join(out, "texture_ktx2_baseColor_default")))
    assert drc == ["%05d.drc" % k for k in range(12)] and ktx == ["00000.ktx2", "00001.ktx2", "00002.ktx2"]
    for k, m in enumerate(meshes):
        got = open(os.path.join(out, "geometry_draco", drc[k]), "rb").read()
        assert got == oracle.drc_encode(m["pos"], m["idx_pos"], m["uv"], m["idx_uv"], m["nrm"], m["idx_nrm"])
    for s in range(3):
        got = open(os.path.join(out, "texture_ktx2_baseColor_default", ktx[s]), "rb").read()
        assert got == oracle.ktx2_encode(texs[5 * s:5 * s + 5])
    man = json.load(open(os.path.join(out, "uvol.json")))
    assert man["geometry"]["targets"]["draco"]["frameCount"] == 12
    t = man["texture"]["targets"]["ktx2"]
    assert (t["sequenceCount"], t["sequenceSize"], t["resolution"]) == (3, 5, [64, 64])
    assert "Frames and frame rates are compatible" in r.stdout
    # every URL the stock player would request resolves to a file uvolenc wrote (node re-statement of the
    # player's template substitution, tests/player_urls.js)
    # (tests/player_urls.py is the same restatement in Python and always runs; the node one runs too where node is installed)
    import shutil, player_urls
    urls = player_urls.resolve(os.path.join(out, "uvol.json"))
    if shutil.which("node"):
        assert urls == json.loads(subprocess.check_output(["node", os.path.join(ROOT, "tests", "player_urls.js"), os.path.join(out, "uvol.json")], text=True))
    assert len(urls["geometry"]) == 12 and len(urls["texture"]) == 3 and urls["batchSize"] == 5
    for rel in urls["geometry"] + urls["texture"]:
        assert os.path.isfile(os.path.join(out, rel)), rel
    assert json.load(open(os.path.join(out, "uvol.encoderpy.json")))["geometry"]["frameCount"] == 12


def test_argv_shims_with_reference_command_lines(oracle, tmp_path):
    """The exact command strings scripts/Encoder.py:260 and :290 build, run through shlex like the reference does."""
    import cli_helpers
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "universal-volumetric_amd"), "all"])
    cfgp, cfg, meshes, texs = cli_helpers.make_sequence(str(tmp_path), n_frames=5, tex=64, batch=5)
    obj = os.path.join(str(tmp_path), "OBJ", "frame_00002.obj"); drc = os.path.join(str(tmp_path), "f.drc")
    cmd = f'{os.path.join(BIN, "draco_encoder")} -i "{obj}" -o "{drc}" -qp 11 -qt 10 -qn 8 -qg 8 -cl 7'
    assert subprocess.call(shlex.split(cmd), stdout=subprocess.DEVNULL) == 0
    m = meshes[2]
    assert open(drc, "rb").read() == oracle.drc_encode(m["pos"], m["idx_pos"], m["uv"], m["idx_uv"], m["nrm"], m["idx_nrm"])
    pat = os.path.join(str(tmp_path), "PNG", "export_%05u.png"); ktx = os.path.join(str(tmp_path), "texture_0000000.ktx2")
    cmd = f'{os.path.join(BIN, "basisu")} -ktx2 -tex_type video -multifile_printf "{pat}" -multifile_num 5 -multifile_first 0 -y_flip -output_file "{ktx}"'
    assert subprocess.call(shlex.split(cmd), stdout=subprocess.DEVNULL) == 0
    assert open(ktx, "rb").read() == oracle.ktx2_encode(texs)
    # failure = non-zero exit code, as scripts/Encoder.py:263 expects
    assert subprocess.call([os.path.join(BIN, "draco_encoder"), "-i", "/nonexistent.obj", "-o", drc], stderr=subprocess.DEVNULL) != 0


def test_uvolenc_targets_uastc_and_shims_flags(oracle, tmp_path):
    """On the GPU: `--targets ktx2,etc2` (raw ETC2 target + two-target manifest), `--uastc`, and the documented flag ranges of the
    shims (`-cl` 1..10 encoded with the cl 7 tool set, `-cl 0` with sequential connectivity, `-uastc`)."""
    import numpy as np
    import cli_helpers, helpers, player_urls
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "universal-volumetric_amd"), "all"])
    cfgp, cfg, meshes, texs = cli_helpers.make_sequence(str(tmp_path), n_frames=7, tex=64, batch=3)
    r = subprocess.run([os.path.join(BIN, "uvolenc"), cfgp, "--targets", "ktx2,etc2", "--batch-frames", "4"], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    out = cfg["OutputDirectory"]
    urls = player_urls.resolve(os.path.join(out, "uvol.json"), supports_etc2=True)
    assert urls["textureTarget"] == "etc2" and len(urls["texture"]) == 7
    for k, rel in enumerate(urls["texture"]):
        raw = np.frombuffer(open(os.path.join(out, rel), "rb").read(), np.uint8)
        ref = oracle.ktx2_decode(open(os.path.join(out, "texture_ktx2_baseColor_default", "%05d.ktx2" % (k // 3)), "rb").read())
        assert np.array_equal(helpers.etc1_decode_blocks(raw.reshape(16, 16, 8), 64, 64), ref.images[k % 3])
    # --uastc: the segments are UASTC KTX2 files, byte-identical with the oracle
    import shutil
    shutil.rmtree(out)
    r = subprocess.run([os.path.join(BIN, "uvolenc"), cfgp, "--uastc"], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    for s, n in enumerate([3, 3, 1]):
        assert open(os.path.join(out, "texture_ktx2_baseColor_default", "%05d.ktx2" % s), "rb").read() == oracle.uastc_ktx2_encode(texs[3 * s:3 * s + n])
    # shims: every documented compression level, and -uastc
    obj = os.path.join(str(tmp_path), "OBJ", "frame_00001.obj"); m = meshes[1]
    want = oracle.drc_encode(m["pos"], m["idx_pos"], m["uv"], m["idx_uv"], m["nrm"], m["idx_nrm"], qp=14, qt=12, qn=10)
    want0 = oracle.drc_encode(m["pos"], m["idx_pos"], m["uv"], m["idx_uv"], m["nrm"], m["idx_nrm"], qp=14, qt=12, qn=10, method=2)
    for cl in (0, 5, 10):                     # level 0 = sequential connectivity (stock draco_encoder's choice), the others the level-7 tool set
        drc = os.path.join(str(tmp_path), "cl%d.drc" % cl)
        assert subprocess.call([os.path.join(BIN, "draco_encoder"), "-i", obj, "-o", drc, "-qp", "14", "-qt", "12", "-qn", "10", "-cl", str(cl)], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL) == 0
        assert open(drc, "rb").read() == (want0 if cl == 0 else want)
    assert subprocess.call([os.path.join(BIN, "draco_encoder"), "-i", obj, "-o", drc, "-cl", "11"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL) != 0
    pat = os.path.join(str(tmp_path), "PNG", "export_%05u.png"); ktx = os.path.join(str(tmp_path), "u.ktx2")
    assert subprocess.call([os.path.join(BIN, "basisu"), "-uastc", "-ktx2", "-tex_type", "video", "-multifile_printf", pat, "-multifile_num", "3", "-multifile_first", "0", "-y_flip", "-output_file", ktx], stdout=subprocess.DEVNULL) == 0
    assert open(ktx, "rb").read() == oracle.uastc_ktx2_encode(texs[:3])


def test_bench_gpus_2_runs_two_ranks(tmp_path):
    """VERDICT r5 item 1 on hardware: `python bench.py --gpus 2` (no launcher) starts two ranks that both encode, the 32-byte manifest
    gather runs, `n_gpus` is the process group's size and the line carries the weak value AND the strong job split over the ranks.
    UVOL_BENCH_ONE_DEVICE=1: both ranks drive device 0 and the collective goes over gloo (this box has one GPU); on a node the same
    command runs one rank per GPU over RCCL."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["UVOL_BENCH_ONE_DEVICE"] = "1"
    argv = ["--gpus", "2", "--steps", "2", "--warmup", "1", "--frames-per-step", "40", "--strong-frames", "60", "--segs", "40", "--rings", "21",
            "--tex-size", "256", "--distinct", "8", "--parity-frames", "4", "--no-cpu-baseline", "--full"]
    import sys
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv, env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    r = lines[0]
    assert r["n_gpus"] == 2 and r["scaling"] == "weak" and r["value"] > 0
    assert r["parity"]["mismatches"] == [] and r["parity"]["geometry_frames_equal_to_oracle"] == 4
    s = r["strong_configs3"]
    assert s["frames_gathered"] == 2 * 60 and s["scaling"] == "strong" and s["frames_per_s"] > 0
