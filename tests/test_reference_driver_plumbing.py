"""BASELINE configs[0]: the STOCK reference driver (scripts/Encoder.py, unmodified, imported from /root/reference)
drives the argv-compatible `draco_encoder` / `basisu` shims over a 10-frame OBJ+PNG sequence.  No GPU here, so the
shims are the test-only builds linked against the hipemu library: this checks the argv / exit-code / file contract
(scripts/Encoder.py:22-42, :260-266, :290-298) and that the outputs are the oracle's bytes."""
import json
import os
import subprocess
import sys
import numpy as np
import pytest
from conftest import ROOT

ENCODER = "/root/reference/scripts/Encoder.py"


@pytest.mark.skipif(not os.path.exists(ENCODER), reason="needs the upstream project's scripts/Encoder.py, which this repository does not carry")
def test_stock_encoder_py_runs_on_shims(oracle, tmp_path):
    import cli_helpers
    pkg = os.path.join(ROOT, "universal-volumetric_amd")
    subprocess.check_call(["make", "-s", "-C", pkg, "hipemu-bins"])
    cfgp, cfg, meshes, texs = cli_helpers.make_sequence(str(tmp_path), n_frames=10, tex=32, batch=5, comments=False)
    env = dict(os.environ)
    env["PATH"] = os.path.join(ROOT, "tests", "hipemu", "bin") + os.pathsep + env["PATH"]          # which() finds the shims first
    env["PYTHONPATH"] = os.path.join(ROOT, "tests", "stubs")
    r = subprocess.run([sys.executable, ENCODER, cfgp], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=900)
    # Both hot loops complete on the shims; the stock driver then dies in its OWN check_total_frames because it sets
    # KTX2FilesPath to the bracketed 'texture_[#######].ktx2', which match_pattern never matches.
    assert "Obtained DRACO files" in r.stdout and "Obtained KTX2 files" in r.stdout, r.stdout + r.stderr
    assert r.returncode != 0 and "IndexError" in r.stderr
    out = cfg["OutputDirectory"]
    drc = sorted(os.listdir(os.path.join(out, "DRC"))); ktx = sorted(os.listdir(os.path.join(out, "KTX2")))
    assert drc == ["frame_%05d.obj.drc" % k for k in range(10)] and ktx == ["texture_0000000.ktx2", "texture_0000001.ktx2"]
    for k, m in enumerate(meshes):
        got = open(os.path.join(out, "DRC", drc[k]), "rb").read()
        assert got == oracle.drc_encode(m["pos"], m["idx_pos"], m["uv"], m["idx_uv"], m["nrm"], m["idx_nrm"])
    for s in range(2):
        got = open(os.path.join(out, "KTX2", ktx[s]), "rb").read()
        assert got == oracle.ktx2_encode(texs[5 * s:5 * s + 5])
    # resume the reference's way (README.md:54-56): hand it the produced files with bare-hash patterns -> accounting + manifest
    cfg2 = {k: v for k, v in cfg.items() if k not in ("OBJFilesPath", "ImagesPath", "KTX2_FIRST_FILE", "KTX2_FILE_COUNT")}
    cfg2["DRACOFilesPath"] = os.path.join(out, "DRC", "frame_#####.obj.drc"); cfg2["KTX2FilesPath"] = os.path.join(out, "KTX2", "texture_#######.ktx2")
    cfgp2 = os.path.join(str(tmp_path), "resume.json"); json.dump(cfg2, open(cfgp2, "w"))
    r2 = subprocess.run([sys.executable, ENCODER, cfgp2], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0, r2.stdout + r2.stderr
    assert "Frames and frame rates are compatible" in r2.stdout
    man = json.load(open(os.path.join(out, "uvol.json")))
    assert man["geometry"]["frameCount"] == 10 and man["texture"]["targets"][0]["sequenceCount"] == 2 and man["texture"]["targets"][0]["sequenceSize"] == 5


def test_shim_exit_codes(tmp_path):
    pkg = os.path.join(ROOT, "universal-volumetric_amd")
    subprocess.check_call(["make", "-s", "-C", pkg, "hipemu-bins"])
    b = os.path.join(ROOT, "tests", "hipemu", "bin")
    assert subprocess.call([os.path.join(b, "draco_encoder"), "-i", str(tmp_path / "missing.obj"), "-o", str(tmp_path / "x.drc")], stderr=subprocess.DEVNULL) != 0
    assert subprocess.call([os.path.join(b, "basisu"), "-ktx2", "-multifile_printf", str(tmp_path / "m_%05u.png"), "-multifile_num", "2", "-output_file", str(tmp_path / "x.ktx2")], stderr=subprocess.DEVNULL) != 0


def test_uvolenc_hipemu_pipeline(oracle, tmp_path):
    """The uvolenc host driver linked against the tests/hipemu build (no GPU): several geometry batches (double-buffered
    parallel OBJ ingest), full texture segments through the batched entry point plus a short last segment, both stages
    running concurrently; every file byte-identical with the oracle and the manifest playable (tests/player_urls.js)."""
    import shutil
    import cli_helpers
    pkg = os.path.join(ROOT, "universal-volumetric_amd")
    subprocess.check_call(["make", "-s", "-C", pkg, "hipemu-bins"])
    cfgp, cfg, meshes, texs = cli_helpers.make_sequence(str(tmp_path), n_frames=7, tex=32, batch=3)
    r = subprocess.run([os.path.join(ROOT, "tests", "hipemu", "bin", "uvolenc"), cfgp, "--batch-frames", "3", "--ingest-threads", "3"],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    out = cfg["OutputDirectory"]
    for k, m in enumerate(meshes):
        got = open(os.path.join(out, "geometry_draco", "%05d.drc" % k), "rb").read()
        assert got == oracle.drc_encode(m["pos"], m["idx_pos"], m["uv"], m["idx_uv"], m["nrm"], m["idx_nrm"])
    for s, n in enumerate([3, 3, 1]):
        got = open(os.path.join(out, "texture_ktx2_baseColor_default", "%05d.ktx2" % s), "rb").read()
        assert got == oracle.ktx2_encode(texs[3 * s:3 * s + n])
    assert r.stdout.index("Obtained DRACO files") < r.stdout.index("Obtained KTX2 files")
    assert shutil.which("node"), "node (>= 12) is part of this container: the player-URL check must run, not be skipped"
    import player_urls
    urls = json.loads(subprocess.check_output(["node", os.path.join(ROOT, "tests", "player_urls.js"), os.path.join(out, "uvol.json")], text=True))
    assert urls == player_urls.resolve(os.path.join(out, "uvol.json"))          # the Python restatement used on the GPU box agrees with the node one
    assert len(urls["geometry"]) == 7 and len(urls["texture"]) == 3
    for rel in urls["geometry"] + urls["texture"]:
        assert os.path.isfile(os.path.join(out, rel)), rel


def test_uvolenc_hipemu_rgba_pngs_get_alpha_slices(oracle, tmp_path):
    """PNGs with an alpha channel through the whole driver: the segments carry alpha slices exactly as the oracle writes
    them (second slice per image, second DFD sample), the manifest is unchanged.  (`--targets ...,etc2` is an opaque format - the
    reference uploads it as RGB_ETC2_Format, src/V2/player.ts:465 - and the transcode entry point it uses refuses such a file:
    tests/test_hipemu_tex.py::test_hipemu_etc1s_alpha_slices.)"""
    import cli_helpers
    pkg = os.path.join(ROOT, "universal-volumetric_amd")
    subprocess.check_call(["make", "-s", "-C", pkg, "hipemu-bins"])
    cfgp, cfg, meshes, texs = cli_helpers.make_sequence(str(tmp_path), n_frames=4, tex=32, batch=2, alpha=True)
    exe = os.path.join(ROOT, "tests", "hipemu", "bin", "uvolenc")
    r = subprocess.run([exe, cfgp, "--batch-frames", "4"], cwd=str(tmp_path), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    out = cfg["OutputDirectory"]
    for s in range(2):
        got = open(os.path.join(out, "texture_ktx2_baseColor_default", "%05d.ktx2" % s), "rb").read()
        assert got == oracle.ktx2_encode(texs[2 * s:2 * s + 2])
        d = oracle.ktx2_decode(got)
        assert d.has_alpha == 1 and d.layers == 2 and d.n_slices == 4


def test_uvolenc_hipemu_targets_etc2_and_multi_gpu_plan(oracle, tmp_path):
    """`--targets ktx2,etc2` (src/Interfaces.ts:19, :60-73): one raw ETC2-RGB block image per frame next to the KTX2
    segments, both targets in the manifest; a renderer with the ETC extension picks `etc2` (src/V2/player.ts:208-222) and every URL
    resolves; the blocks decode (independent ETC1 decoder of tests/helpers.py) to the RGBA decode of the segment.  `--gpus 2` on
    the one emulated device exercises the segment-aligned frame blocks of shard_plan (same files as one GPU)."""
    import shutil
    import numpy as np
    import cli_helpers, helpers, player_urls
    pkg = os.path.join(ROOT, "universal-volumetric_amd")
    subprocess.check_call(["make", "-s", "-C", pkg, "hipemu-bins"])
    cfgp, cfg, meshes, texs = cli_helpers.make_sequence(str(tmp_path), n_frames=7, tex=32, batch=3)
    r = subprocess.run([os.path.join(ROOT, "tests", "hipemu", "bin", "uvolenc"), cfgp, "--batch-frames", "3", "--targets", "ktx2,etc2"],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    out = cfg["OutputDirectory"]
    man = json.load(open(os.path.join(out, "uvol.json")))
    assert set(man["texture"]["targets"]) == {"ktx2", "etc2"}
    e = man["texture"]["targets"]["etc2"]
    assert (e["format"], e["sequenceSize"], e["sequenceCount"], e["resolution"], e["frameRate"]) == ("etc2", 1, 7, [32, 32], 30)
    for supports, want in ((False, "ktx2"), (True, "etc2")):
        urls = player_urls.resolve(os.path.join(out, "uvol.json"), supports_etc2=supports)
        assert urls["textureTarget"] == want
        if shutil.which("node"):
            js = json.loads(subprocess.check_output(["node", os.path.join(ROOT, "tests", "player_urls.js"), os.path.join(out, "uvol.json")] + (["--supports", "etc2"] if supports else []), text=True))
            assert js == urls
        for rel in urls["geometry"] + urls["texture"]:
            assert os.path.isfile(os.path.join(out, rel)), rel
    assert urls["texture"] == ["texture_etc2_baseColor_default/%05d.etc2" % k for k in range(7)] and urls["batchSize"] == 1
    for s, n in enumerate([3, 3, 1]):
        ref = oracle.ktx2_decode(open(os.path.join(out, "texture_ktx2_baseColor_default", "%05d.ktx2" % s), "rb").read())
        for l in range(n):
            raw = np.frombuffer(open(os.path.join(out, "texture_etc2_baseColor_default", "%05d.etc2" % (3 * s + l)), "rb").read(), np.uint8)
            assert raw.size == 8 * 8 * 8
            assert np.array_equal(helpers.etc1_decode_blocks(raw.reshape(8, 8, 8), 32, 32), ref.images[l])
    # the plan itself (uvolenc --gpus N > 1 runs end to end in test_uvolenc_hipemu_gpus_2_and_8_write_what_one_gpu_writes)
    import ctypes as C
    L = C.CDLL(os.path.join(pkg, "libuvolhost.so"))
    L.uvolh_shard_plan.argtypes = [C.c_long, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_long)]
    import shard
    for n, b, w in [(1200, 5, 8), (7, 3, 2), (13, 5, 8), (10, 7, 3)]:
        for rk in range(w):
            o4 = (C.c_long * 4)(); L.uvolh_shard_plan(n, b, w, rk, o4)
            assert tuple(o4) == tuple(shard.plan(n, b, w, rk))


def test_uvolenc_hipemu_gpus_2_and_8_write_what_one_gpu_writes(oracle, tmp_path):
    """the multi-device host path of uvolenc (one thread and one context pair per device, segment-aligned blocks of
    frames per device, scripts/Encoder.py:103-154 accounting) executed with N > 1 - on the emulation's HIPEMU_DEVICES - must write
    exactly the files and the manifest that --gpus 1 writes: 7 frames, KTX2_BATCH_SIZE 3 (a short last segment, fewer segments than
    devices for N = 8 so some devices get nothing)."""
    import filecmp, cli_helpers
    pkg = os.path.join(ROOT, "universal-volumetric_amd")
    subprocess.check_call(["make", "-s", "-C", pkg, "hipemu-bins"])
    exe = os.path.join(ROOT, "tests", "hipemu", "bin", "uvolenc")
    outs = {}
    for gpus in (1, 2, 8):
        root = str(tmp_path / ("g%d" % gpus)); os.makedirs(root)
        cfgp, cfg, meshes, texs = cli_helpers.make_sequence(root, n_frames=7, tex=32, batch=3)
        r = subprocess.run([exe, cfgp, "--batch-frames", "4", "--gpus", str(gpus)], cwd=root, capture_output=True, text=True, timeout=900,
                           env=dict(os.environ, HIPEMU_DEVICES="8"))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs[gpus] = cfg["OutputDirectory"]
    ref = outs[1]
    names = sorted(os.path.relpath(os.path.join(d, f), ref) for d, _, fs in os.walk(ref) for f in fs)
    assert len([n for n in names if n.endswith(".drc")]) == 7 and len([n for n in names if n.endswith(".ktx2")]) == 3
    for gpus in (2, 8):
        got = sorted(os.path.relpath(os.path.join(d, f), outs[gpus]) for d, _, fs in os.walk(outs[gpus]) for f in fs)
        assert got == names, (gpus, set(got) ^ set(names))
        for n in names:
            if n.endswith("uvol.json"):
                a, b = json.load(open(os.path.join(ref, n))), json.load(open(os.path.join(outs[gpus], n)))
                assert a == b, (gpus, n)
            else:
                assert filecmp.cmp(os.path.join(ref, n), os.path.join(outs[gpus], n), shallow=False), (gpus, n)
    # and what one device wrote is what the oracle writes
    m0 = cli_helpers.make_sequence(str(tmp_path / "chk"), n_frames=1, tex=32, batch=3)[2][0]
    assert open(os.path.join(ref, "geometry_draco", "00000.drc"), "rb").read() == oracle.drc_encode(m0["pos"], m0["idx_pos"], m0["uv"], m0["idx_uv"], m0["nrm"], m0["idx_nrm"])


def test_uvolenc_hipemu_device_inflate_writes_the_same_files(oracle, tmp_path):
    """VERDICT r4 item 6a in the pipeline: `uvolenc --device-inflate` hands the PNGs' zlib streams to uvol_inflate_png_batch_dev instead
    of inflating them on the ingest threads; every .ktx2 / .drc / manifest byte equals the default run's; a PNG whose IDAT data is
    corrupt fails its segment with the reference's message (scripts/Encoder.py:293-298) and a non-zero exit."""
    import filecmp, glob, zlib, struct, cli_helpers
    pkg = os.path.join(ROOT, "universal-volumetric_amd")
    subprocess.check_call(["make", "-s", "-C", pkg, "hipemu-bins"])
    exe = os.path.join(ROOT, "tests", "hipemu", "bin", "uvolenc")
    outs = {}
    for name, extra in (("host", []), ("dev", ["--device-inflate", "--tex-batch-frames", "4", "--pinned-text"])):      # (--pinned-text: OBJ files read into a page-locked slab)
        root = str(tmp_path / name); os.makedirs(root)
        cfgp, cfg, meshes, texs = cli_helpers.make_sequence(root, n_frames=4, tex=32, batch=2)
        r = subprocess.run([exe, cfgp, "--batch-frames", "4"] + extra, cwd=root, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs[name] = cfg["OutputDirectory"]
    names = sorted(os.path.relpath(os.path.join(d, f), outs["host"]) for d, _, fs in os.walk(outs["host"]) for f in fs)
    assert len([n for n in names if n.endswith(".ktx2")]) == 2
    for n in names:
        if n.endswith("uvol.json"):
            assert json.load(open(os.path.join(outs["host"], n))) == json.load(open(os.path.join(outs["dev"], n)))
        else:
            assert filecmp.cmp(os.path.join(outs["host"], n), os.path.join(outs["dev"], n), shallow=False), n
    # corrupt the image data of one PNG of the second segment (chunk layout kept; the host parser does not look at CRCs)
    root = str(tmp_path / "bad"); os.makedirs(root)
    cfgp, cfg, meshes, texs = cli_helpers.make_sequence(root, n_frames=4, tex=32, batch=2)
    pngs = sorted(glob.glob(os.path.join(root, "**", "*.png"), recursive=True)); assert len(pngs) == 4
    d = bytearray(open(pngs[2], "rb").read()); o = d.find(b"IDAT"); assert o > 0
    ln = struct.unpack(">I", d[o - 4:o])[0]; d[o + 4 + ln // 2] ^= 0x3c; d[o + 4 + ln // 2 + 1] ^= 0xc3
    open(pngs[2], "wb").write(d)
    r = subprocess.run([exe, cfgp, "--batch-frames", "4", "--device-inflate"], cwd=root, capture_output=True, text=True, timeout=900)
    assert r.returncode != 0 and "Failed to compress images with indices" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_audio_duration_probe(tmp_path):
    """scripts/Encoder.py:331-347 compares the audio duration with the geometry / texture durations; uvolenc probes WAV and MP3
    files itself (no audioread here): a PCM WAV of known length and a synthetic CBR MPEG-1 Layer III stream behind an ID3v2 tag."""
    import ctypes as C, struct, wave
    pkg = os.path.join(ROOT, "universal-volumetric_amd")
    subprocess.check_call(["make", "-s", "-C", pkg, "libuvolhost.so"])
    L = C.CDLL(os.path.join(pkg, "libuvolhost.so")); L.uvolh_audio_duration.restype = C.c_double; L.uvolh_audio_duration.argtypes = [C.c_char_p]
    w = wave.open(str(tmp_path / "a.wav"), "wb"); w.setnchannels(2); w.setsampwidth(2); w.setframerate(48000); w.writeframes(b"\0" * (4 * 48000 * 3)); w.close()
    assert abs(L.uvolh_audio_duration(str(tmp_path / "a.wav").encode()) - 3.0) < 1e-9
    # 100 frames, MPEG-1 Layer III, 128 kbit/s, 44.1 kHz, no padding: 417 bytes and 1152 samples each
    hdr = bytes([0xFF, 0xFB, 0x90, 0x00]); frame = hdr + b"\0" * (417 - 4)
    (tmp_path / "a.mp3").write_bytes(b"ID3\x03\x00\x00\x00\x00\x00\x0a" + b"\0" * 10 + frame * 100)
    assert abs(L.uvolh_audio_duration(str(tmp_path / "a.mp3").encode()) - 100 * 1152 / 44100) < 1e-9
    assert L.uvolh_audio_duration(str(tmp_path / "missing.mp3").encode()) < 0
