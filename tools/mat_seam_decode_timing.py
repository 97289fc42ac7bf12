#!/usr/bin/env python3
"""What decoding the corner-form material attribute costs the files that do not carry one, and what it costs the files that do, on a real
GPU.  N frames of the bench's shape per call (the bench's mesh generator, four distinct frames cycled, encoded by the library without ids:
what bench.py's decode step reads), three calls per child process:
  decode_mesh   uvol_decode_mesh_batch, results left in HBM - bench.py's `decode_mesh` measurement, call for call
  mat           uvol_decode_mesh_batch_mat with has_material, arrays left in HBM (no file carries a corner material: the third table's pass is not enqueued)
  packed        uvol_decode_mesh_batch_packed, device outputs (the same)
this build and another build of the library (the parent commit's) alternated in fresh child processes, two runs each.  Then, this build
alone: the same sphere with ids in four latitude bands, encoded with material_seams = 1 (a slot-2 corner material: the pass does run), `mat`
and `packed` with the pass's group time.  Writes profiles/r12_material_seam_decode.json.

usage: tools/mat_seam_decode_timing.py [n_frames] --parent-lib PATH [--runs 2] [--seamed-frames 960] [--out FILE]   (driver: never opens the GPU)
       tools/mat_seam_decode_timing.py [n_frames] --child plain|seamed [--lib PATH]                                (one process, one JSON line)"""
import argparse, ctypes as C, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "universal-volumetric_amd"))
REPEATS = 3
PASS_GROUP = "geodec.k7b_material_table"
SHAPE = tuple(int(x) for x in os.environ.get("UVOL_TIMING_SHAPE", "400,251").split(","))      # sphere segments, rings (default: the bench's 100,002 vertices)


def four_bands(m):
    """One id per face: four latitude bands (the sphere's polar axis is y)."""
    import numpy as np
    y = np.asarray(m["pos"], np.float64).reshape(-1, 3)[np.asarray(m["idx_pos"], np.int64).reshape(-1, 3)].mean(1)[:, 1]
    return np.minimum(((y - y.min()) / (np.ptp(y) + 1e-9) * 4).astype(np.int64), 3).astype(np.uint8)


def child(n, kind, lib):
    import numpy as np, synth, uvol
    from points_timing import Hbm
    seamed = kind == "seamed"
    c = uvol.Codec(device=0, max_batch=n, lib_path=lib, **(dict(material_seams=1) if seamed else {}))
    meshes = [synth.sphere_mesh(*SHAPE, frame=k, seed=k) for k in range(4)]
    distinct = c.encode_mesh_batch([dict(m, face_mat=four_bands(m)) for m in meshes] if seamed else meshes)
    files = [distinct[i % 4] for i in range(n)]
    nfs = [c.drc_info(f)[0] for f in distinct]
    pk4 = c.decode_mesh_batch_packed(distinct)
    pts = [r["n_points"] for r in pk4]
    res = dict(kind=kind, frames=n, lib=os.path.basename(os.path.dirname(os.path.dirname(lib))) if lib else "this build", faces_per_frame=nfs, points_per_frame=pts,
               has_material=[int(r["has_material"]) for r in pk4], file_bytes=[len(f) for f in distinct])
    fp = (C.c_char_p * n)(*files); ln = (C.c_size_t * n)(*[len(f) for f in files]); st = (C.c_int * n)(); hm = (C.c_int * n)()
    dm = (uvol.DecodedMesh * n)(); pm = (uvol.PackedPoints * n)()
    total = sum(512 + 16 * pts[i % 4] + 12 * nfs[i % 4] for i in range(n)) + 4096
    if lib and "hipemu" in lib:                                              # rehearsal without a GPU: the emulation's device memory is host memory
        class HostMem:
            def __init__(self, nb): self.a = np.zeros(nb + 256, np.uint8); self.off = -self.a.ctypes.data % 256
            def take(self, nb): o = (self.off + 255) & ~255; self.off = o + nb; return self.a.ctypes.data + o
            def free(self): pass
        mem = HostMem(total)
    else: mem = Hbm(total)
    for i in range(n):
        dm[i].cap_faces = pm[i].cap_faces = nfs[i % 4]; dm[i].cap_values = 3 * nfs[i % 4]; pm[i].cap_points = pts[i % 4]
        pm[i].records = mem.take(16 * pts[i % 4]); pm[i].index = mem.take(12 * nfs[i % 4])
    runs = [("mat", lambda: c.L.uvol_decode_mesh_batch_mat(c.h, fp, ln, n, 0, dm, None, hm, st)),
            ("packed", lambda: c.L.uvol_decode_mesh_batch_packed(c.h, fp, ln, n, 1, pm, st))]
    if not seamed: runs.insert(0, ("decode_mesh", lambda: c.L.uvol_decode_mesh_batch(c.h, fp, ln, n, dm, st)))
    for name, run in runs:
        assert run() == 0 and list(st) == [0] * n, (name, list(st)[:8], c.error())      # warm-up: allocates the workspaces of the whole batch
        if name == "mat": assert list(hm) == [1 if seamed else 0] * n
        ms = []
        for _ in range(REPEATS):
            t = time.perf_counter(); rc = run(); ms.append(1000 * (time.perf_counter() - t)); assert rc == 0
        c.profile(True); c.profile_reset(); run()
        groups = {g["name"]: round(g["total_ms"], 2) for g in c.profile_report() if g["launches"]}
        c.profile(False)
        res[name] = dict(frames_per_s=n / (min(ms) / 1000), ms_calls=[round(x, 2) for x in ms], groups_ms=groups)
    mem.free(); c.close()
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser(); ap.add_argument("n", nargs="?", type=int, default=1920); ap.add_argument("--child"); ap.add_argument("--lib")
    ap.add_argument("--parent-lib"); ap.add_argument("--runs", type=int, default=2); ap.add_argument("--seamed-frames", type=int, default=960); ap.add_argument("--out")
    a = ap.parse_args()
    if a.child:
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        return child(a.n, a.child, a.lib)
    a.out = a.out or os.path.join(ROOT, "profiles", "r12_material_seam_decode.json")
    out = dict(frames_per_call=a.n, repeats_per_process=REPEATS, runs=[], note="fresh processes, parent build / this build alternated; frames_per_s is the best of ms_calls; "
               "groups_ms are the library's event brackets of one further call")
    def one(kind, lib, n):
        cmd = [sys.executable, os.path.abspath(__file__), str(n), "--child", kind] + (["--lib", lib] if lib else [])
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=420)
        if r.returncode != 0:
            raise SystemExit("child %s failed (%d): %s" % (kind, r.returncode, r.stderr[-2000:]))      # nothing more is started after a failure
        return json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    for k in range(a.runs):
        rnd = dict(parent=one("plain", a.parent_lib, a.n), this=one("plain", None, a.n))
        out["runs"].append(rnd)
        print(json.dumps({who: {nm: round(v["frames_per_s"], 1) for nm, v in p.items() if isinstance(v, dict)} for who, p in rnd.items()}), flush=True)
        json.dump(out, open(a.out, "w"), indent=1)
    out["seamed_four_bands"] = one("seamed", None, a.seamed_frames)
    s = out["seamed_four_bands"]
    print(json.dumps({nm: dict(frames_per_s=round(s[nm]["frames_per_s"], 1), pass_ms=s[nm]["groups_ms"].get(PASS_GROUP)) for nm in ("mat", "packed")}), flush=True)
    # the margin: this build's slower run may fall below the parent's slower run by no more than the parent's own spread
    gate = {}
    for nm in ("decode_mesh", "mat", "packed"):
        p = sorted(r["parent"][nm]["frames_per_s"] for r in out["runs"]); t = sorted(r["this"][nm]["frames_per_s"] for r in out["runs"])
        gate[nm] = dict(parent=[round(x, 1) for x in p], this=[round(x, 1) for x in t], parent_spread=round(p[-1] - p[0], 1), within=bool(t[0] >= p[0] - (p[-1] - p[0])))
    out["margin"] = gate
    print(json.dumps(gate), flush=True)
    json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
