#!/usr/bin/env python3
"""tools/jpeg_timing.py [layers=64] [size=2048] [runs=3] [--e2e DIR FRAMES]: the JPEG ingest on the MI355X.

Kernel: `layers` images of size x size at 4:2:0, made by tiling the coefficients of a fixture (tests/golden/jpeg/seq_2.jpg), through one
profiled uvol_idct_jpeg_batch_dev call per run; the groups jpeg.upload / jpeg.idct from uvol_profile_get.  The first and the last layer are
compared with the NumPy restatement of the rule (tests/jpeg_cases.py), so every round of the kernels' grid-stride loops is checked at this
size.  Beside it, for orientation, ingest.png_unfilter for the same number of RGBA layers of that size.

--e2e DIR FRAMES: writes FRAMES 100,002-vertex OBJ files and the same FRAMES textures once as JPEG (quality 90, 4:2:0) and once as PNG, runs
`uvolenc` (UVOL_TIMING=1) on each and prints the end-to-end frames/s and the [uvolenc-timing] load lines.  Needs Pillow."""
import json, os, re, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "universal-volumetric_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import uvol, jpeg_cases as JC, material_cases as MC

args = [a for a in sys.argv[1:]]
e2e = None
if "--e2e" in args:
    k = args.index("--e2e"); e2e = (args[k + 1], int(args[k + 2])); del args[k:k + 3]
layers = int(args[0]) if len(args) > 0 else 64; size = int(args[1]) if len(args) > 1 else 2048; runs = int(args[2]) if len(args) > 2 else 3


def groups(cd):
    return {g["name"]: g for g in cd.profile_report()}


def kernel_timing():
    P, _ = JC.reference("seq_2")                                  # 24 x 24, 4:2:0: luma 4 x 4 blocks (the 3 x 3 real ones + padding), chroma 2 x 2
    assert size % 16 == 0
    by, bc = size // 8, size // 16
    Y = P.coef[:16 * 64].reshape(4, 4, 64)[:3, :3]; Cb = P.coef[16 * 64:20 * 64].reshape(2, 2, 64)[:1, :1]; Cr = P.coef[20 * 64:].reshape(2, 2, 64)[:1, :1]
    tile = lambda g, n: np.tile(g, (-(-n // g.shape[0]), -(-n // g.shape[1]), 1))[:n, :n]
    coef = np.ascontiguousarray(np.concatenate([tile(Y, by).reshape(-1), tile(Cb, bc).reshape(-1), tile(Cr, bc).reshape(-1)]))
    cd = uvol.Codec(device=0); mem = MC.HipMem()
    assert cd.jpeg_coeff_count(size, size, 3, 2, 2) == coef.size
    out = {"what": "%d layers of %d x %d at 4:2:0, one uvol_idct_jpeg_batch_dev call" % (layers, size, size), "runs": []}
    cd.idct_jpeg_batch_dev([coef] * layers, [P.qt] * layers, size, size, 3, 2, 2)      # warm-up: allocations
    cd.profile(True)
    for r in range(runs):
        cd.profile_reset()
        ptrs = cd.idct_jpeg_batch_dev([coef] * layers, [P.qt] * layers, size, size, 3, 2, 2, slot=r & 1)
        g = groups(cd)
        out["runs"].append({"jpeg.idct_ms": g["jpeg.idct"]["total_ms"], "jpeg.upload_ms": g["jpeg.upload"]["total_ms"], "idct_algo_bytes": g["jpeg.idct"]["algo_bytes"]})
    want = JC.decode(size, size, 3, 2, 2, coef, P.qt)
    for i in (0, layers - 1):
        got = mem.to_host(ptrs[i], np.uint8, size * size * 4).reshape(size, size, 4)
        assert np.array_equal(got, want), "layer %d differs from the rule" % i
    out["bit_exact_layers_checked"] = [0, layers - 1]
    best = min(x["jpeg.idct_ms"] for x in out["runs"]); ab = out["runs"][0]["idct_algo_bytes"]
    out["best_idct_ms"] = best; out["coefficients_plus_rgba_TB_per_s"] = ab / best / 1e9
    # orientation: the PNG un-filter of as many RGBA layers of this size (filter type 0 rows; the kernel's time does not depend on the filter)
    raw = np.zeros((size, 1 + size * 4), np.uint8); raw[:, 1:] = np.arange(size * 4, dtype=np.uint32).astype(np.uint8)[None, :]
    rb = raw.tobytes()
    cd.unfilter_png_batch_dev([rb] * layers, size, size, 4)
    cd.profile_reset()
    cd.unfilter_png_batch_dev([rb] * layers, size, size, 4)
    out["png_unfilter_ms_same_layers"] = groups(cd)["ingest.png_unfilter"]["total_ms"]
    cd.close()
    print(json.dumps(out))


def end_to_end(root, n):
    import synth
    from PIL import Image
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    os.makedirs(os.path.join(root, "OBJ"), exist_ok=True)
    meshes = [synth.sphere_mesh(frame=k, seed=k) for k in range(4)]
    texs = synth.texture_sequence(5, size=size, seed=0)
    for k, m in enumerate(meshes):
        ip, iu, inn = (m[q].reshape(-1, 3).astype(np.int64) + 1 for q in ("idx_pos", "idx_uv", "idx_nrm"))
        with open(os.path.join(root, "OBJ", "src_%d.obj" % k), "w") as f:
            f.write("\n".join("v %.6f %.6f %.6f" % tuple(v) for v in m["pos"].tolist())); f.write("\n")
            f.write("\n".join("vt %.7f %.7f" % tuple(v) for v in m["uv"].tolist())); f.write("\n")
            f.write("\n".join("vn %.6f %.6f %.6f" % tuple(v) for v in m["nrm"].tolist())); f.write("\n")
            f.write("\n".join("f %d/%d/%d %d/%d/%d %d/%d/%d" % tuple(r) for r in np.stack([ip, iu, inn], -1).reshape(-1, 9).tolist())); f.write("\n")
    for k in range(n):
        subprocess.check_call(["cp", os.path.join(root, "OBJ", "src_%d.obj" % (k % 4)), os.path.join(root, "OBJ", "frame_%05d.obj" % k)])
    for kind in ("jpg", "png"):
        d = os.path.join(root, kind.upper()); os.makedirs(d, exist_ok=True)
        for k in range(5):
            if kind == "jpg":
                Image.fromarray(texs[k][..., :3]).save(os.path.join(d, "src_%d.jpg" % k), quality=90, subsampling=2)
            else:
                Image.fromarray(texs[k], "RGBA").save(os.path.join(d, "src_%d.png" % k), compress_level=1)
        for k in range(n):
            subprocess.check_call(["cp", os.path.join(d, "src_%d.%s" % (k % 5, kind)), os.path.join(d, "export_%05d.%s" % (k, kind))])
        cfg = {"name": "e2e", "OBJFilesPath": os.path.join(root, "OBJ", "frame_#####.obj"), "ImagesPath": os.path.join(d, "export_#####." + kind),
               "KTX2_FIRST_FILE": 0, "KTX2_FILE_COUNT": n, "KTX2_BATCH_SIZE": 5, "GEOMETRY_FRAME_RATE": 30, "TEXTURE_FRAME_RATE": 30, "OutputDirectory": os.path.join(root, "out_" + kind)}
        cfgp = os.path.join(root, "project-config-%s.json" % kind); json.dump(cfg, open(cfgp, "w"))
        t = time.perf_counter()
        r = subprocess.run([os.path.join(ROOT, "universal-volumetric_amd", "bin", "uvolenc"), cfgp, "--batch-frames", str(min(n, 120))], cwd=root, capture_output=True, text=True,
                           env=dict(os.environ, UVOL_TIMING="1"), timeout=600)
        wall = time.perf_counter() - t
        m = re.search(r"encode phase ([0-9.]+) s, ([0-9.]+) frames/s", r.stdout)
        print(json.dumps({"what": "uvolenc end to end, %d frames, textures as %s (%.2f MB each)" % (n, kind, os.path.getsize(os.path.join(d, "export_00000." + kind)) / 1e6), "rc": r.returncode,
                          "frames_per_s_encode_phase": float(m.group(2)) if m else None, "frames_per_s_process_wall": n / wall,
                          "tex_load_lines": [l for l in r.stderr.splitlines() if "tex load" in l], "tail": r.stdout[-300:] if r.returncode else ""}))


if e2e:
    end_to_end(*e2e)
else:
    kernel_timing()
