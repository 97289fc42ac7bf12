#!/usr/bin/env python3
"""Cost of the render-ready mesh decode on a real GPU: uvol_decode_mesh_batch_points (device outputs, both layouts) against
uvol_decode_mesh_batch_dev of this build and of another build of the library (the parent commit's), N frames of the bench's shape per call,
the three alternated in fresh child processes; every child times REPEATS calls after a warm-up.  Then the weld kernels under
`rocprofv3 --kernel-trace --stats` and, each in a pass of its own, under `--pmc FETCH_SIZE` and `--pmc WRITE_SIZE` (fewer frames: the
counters serialise the kernels).  Writes profiles/r08_points_decode.json.

--packed: uvol_decode_mesh_batch_packed (16-byte integer records) against the float interleaved form of this build and of the parent build,
to three destinations - HBM, pageable host arrays, arrays in uvol_host_alloc memory -, alternated in fresh child processes in the same
session; the output arrays are allocated and touched once per process, outside the timed calls.  Writes profiles/r07_packed_points.json.

usage: tools/points_timing.py [n_frames] --parent-lib PATH [--pairs 3] [--prof-frames 240] [--out FILE]   (driver: starts the children, never opens the GPU)
       tools/points_timing.py [n_frames] --packed --parent-lib PATH [--pairs 3] [--out FILE]               (driver of the packed comparison)
       tools/points_timing.py [n_frames] --child points|dev|packed [--dest dev|host|pinned] [--lib PATH]  (one measurement, one JSON line)"""
import argparse, collections, csv, ctypes as C, glob, json, os, re, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "universal-volumetric_amd"))
REPEATS = 5


class Hbm:
    """One hipMalloc, carved 256-byte aligned."""
    def __init__(self, nbytes):
        self.hip = C.CDLL("libamdhip64.so"); p = C.c_void_p()
        if self.hip.hipMalloc(C.byref(p), C.c_size_t(nbytes)) != 0: raise RuntimeError("hipMalloc(%d) failed" % nbytes)
        self.base, self.off, self.n = p.value, 0, nbytes

    def take(self, nbytes):
        o = (self.off + 255) & ~255; assert o + nbytes <= self.n; self.off = o + nbytes; return self.base + o

    def free(self):
        self.hip.hipFree(C.c_void_p(self.base))


def child(n, mode, lib):
    import numpy as np, synth, uvol
    c = uvol.Codec(device=0, max_batch=n, lib_path=lib)
    distinct = c.encode_mesh_batch([synth.sphere_mesh(frame=k) for k in range(4)])
    files = [distinct[i % 4] for i in range(n)]
    probe = c.decode_mesh_batch(distinct, fetch=False)                     # counts of the four distinct frames: the buffers below are sized exactly
    res = dict(mode=mode, frames=n, lib=os.path.basename(os.path.dirname(lib)) if lib else "this build")
    if mode == "dev":
        per = [sum(256 + 4 * w * p[k] for k, w in (("n_pos", 3), ("n_uv", 2), ("n_nrm", 3))) + 3 * (256 + 12 * p["n_faces"]) for p in probe]
        mem = Hbm(sum(per[i % 4] for i in range(n)) + 4096)
        metas = (uvol.DecodedMesh * n)()
        for i in range(n):
            p = probe[i % 4]; m = metas[i]; m.cap_faces = p["n_faces"]; m.cap_values = 3 * p["n_faces"]
            m.pos, m.uv, m.nrm = mem.take(12 * p["n_pos"]), mem.take(8 * p["n_uv"]), mem.take(12 * p["n_nrm"])
            m.idx_pos, m.idx_uv, m.idx_nrm = (mem.take(12 * p["n_faces"]) for _ in range(3))
        run = lambda: c.decode_mesh_batch_dev(files, metas)
        runs = [("dev", run)]
    else:
        pts = [r["n_points"] for r in c.decode_mesh_batch_points(distinct)]
        mem = Hbm(sum(512 + 32 * pts[i % 4] + 12 * probe[i % 4]["n_faces"] for i in range(n)) + 4096)
        metas = (uvol.DecodedPoints * n)()
        for i in range(n):
            m = metas[i]; m.cap_faces = probe[i % 4]["n_faces"]; m.cap_points = pts[i % 4]
            m.pos = mem.take(32 * pts[i % 4]); m.index = mem.take(12 * probe[i % 4]["n_faces"])      # (planar: pos only fills 12 of the 32 bytes; uv / nrm skipped below)
        res["points_per_frame"] = pts; res["corners_per_frame"] = [3 * p["n_faces"] for p in probe]; res["pos_entries_per_frame"] = [p["n_pos"] for p in probe]
        def mk(layout):
            def run():
                if layout == "planar":                                      # planar into the same memory: pos | nrm | uv blocks of the frame's buffer
                    for i in range(n):
                        m = metas[i]; m.nrm = m.pos + 12 * pts[i % 4]; m.uv = m.pos + 24 * pts[i % 4]
                return c.decode_mesh_batch_points(files, layout=layout, on_device=True, metas=metas)
            return run
        runs = [("interleaved", mk("interleaved")), ("planar", mk("planar"))]
    for name, run in runs:
        st = run(); assert st == [0] * n, st[:8]                            # warm-up: allocates the workspaces of the whole batch
        ms = []
        for _ in range(REPEATS):                                            # without the event brackets
            t = time.perf_counter(); run(); ms.append(1000 * (time.perf_counter() - t))
        c.profile(True); c.profile_reset()
        t = time.perf_counter(); run(); dt = time.perf_counter() - t
        groups = {g["name"]: round(g["total_ms"], 2) for g in c.profile_report() if g["launches"]}
        c.profile(False)
        best = min(ms)
        res[name] = dict(frames_per_s=n / (best / 1000), ms_best=best, ms_calls=[round(x, 2) for x in ms], frames_per_s_bracketed=n / dt, groups_ms=groups)
    if mode == "points":
        corners = sum(res["corners_per_frame"][i % 4] for i in range(n)); points = sum(pts[i % 4] for i in range(n))
        res["weld_compulsory_bytes"] = 16 * corners + 32 * points          # 12 read + 4 written per corner, 32 per point
    mem.free(); c.close()
    print("RESULT " + json.dumps(res))


def child_packed(n, dest, lib):
    """Float interleaved records and, where the library has it, packed records of n frames into `dest` memory."""
    import numpy as np, synth, uvol
    c = uvol.Codec(device=0, max_batch=n, lib_path=lib)
    distinct = c.encode_mesh_batch([synth.sphere_mesh(frame=k) for k in range(4)])
    files = [distinct[i % 4] for i in range(n)]
    nfs = [c.drc_info(f)[0] for f in distinct]; pts = [r["n_points"] for r in c.decode_mesh_batch_points(distinct)]
    has_packed = hasattr(c.L, "uvol_decode_mesh_batch_packed")
    fp = (C.c_char_p * n)(*files); ln = (C.c_size_t * n)(*[len(f) for f in files]); st = (C.c_int * n)()
    total = sum(512 + 32 * pts[i % 4] + 12 * nfs[i % 4] for i in range(n)) + 4096
    if dest == "dev": mem = Hbm(total); take = mem.take
    elif dest == "pinned": mem = uvol.PinnedArena(total, lib_path=lib); take = lambda nb: mem.take((nb,), np.uint8).ctypes.data
    else:
        keep = []
        def take(nb):
            a = np.zeros(nb, np.uint8); keep.append(a); return a.ctypes.data      # (zeros: every page is touched before the first timed call)
    res = dict(mode="packed", dest=dest, frames=n, lib=os.path.basename(os.path.dirname(lib)) if lib else "this build", points_per_frame=pts, faces_per_frame=nfs)
    bufs = [(take(32 * pts[i % 4]), take(12 * nfs[i % 4])) for i in range(n)]      # the packed form writes the first half of the same record buffers
    fm = (uvol.DecodedPoints * n)(); pm = (uvol.PackedPoints * n)()
    for i in range(n):
        fm[i].cap_faces = pm[i].cap_faces = nfs[i % 4]; fm[i].cap_points = pm[i].cap_points = pts[i % 4]; fm[i].layout = uvol.UVOL_POINTS_INTERLEAVED
        fm[i].pos = pm[i].records = bufs[i][0]; fm[i].index = pm[i].index = bufs[i][1]
    on_dev = 1 if dest == "dev" else 0
    runs = [("interleaved", lambda: c.L.uvol_decode_mesh_batch_points(c.h, fp, ln, n, on_dev, fm, st), sum(32 * pts[i % 4] + 12 * nfs[i % 4] for i in range(n)))]
    if has_packed: runs.append(("packed", lambda: c.L.uvol_decode_mesh_batch_packed(c.h, fp, ln, n, on_dev, pm, st), sum(16 * pts[i % 4] + 12 * nfs[i % 4] for i in range(n))))
    for name, run, nbytes in runs:
        assert run() == 0 and list(st) == [0] * n, (name, list(st)[:8])       # warm-up: allocates the workspaces of the whole batch
        ms = []
        for _ in range(REPEATS):
            t = time.perf_counter(); rc = run(); ms.append(1000 * (time.perf_counter() - t)); assert rc == 0
        c.profile(True); c.profile_reset(); run()
        groups = {g["name"]: round(g["total_ms"], 2) for g in c.profile_report() if g["launches"]}
        c.profile(False)
        res[name] = dict(frames_per_s=n / (min(ms) / 1000), frames_per_s_calls=[round(n / (x / 1000), 1) for x in ms], ms_calls=[round(x, 2) for x in ms], output_bytes_per_call=nbytes, groups_ms=groups)
    if dest == "dev": mem.free()
    elif dest == "pinned": mem.close()
    c.close()
    print("RESULT " + json.dumps(res))


def main_packed(a):
    out = dict(frames_per_call=a.n, repeats_per_process=REPEATS, rounds=[], note="alternated in fresh processes, per destination: this build (float interleaved records, "
               "then packed records) / the parent build (float interleaved records); frames_per_s is the best of the process's calls, frames_per_s_calls all of them")
    for k in range(a.pairs):
        rnd = {}
        for dest in ("dev", "host", "pinned"):
            for who, lib in (("this", None), ("parent", a.parent_lib)):
                cmd = [sys.executable, os.path.abspath(__file__), str(a.n), "--child", "packed", "--dest", dest] + (["--lib", lib] if lib else [])
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
                if r.returncode != 0:
                    raise SystemExit("child %s/%s failed (%d): %s" % (dest, who, r.returncode, r.stderr[-2000:]))      # nothing more is started after a failure
                rnd[dest + "_" + who] = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
        out["rounds"].append(rnd)
        print(json.dumps({k2: {nm: round(v["frames_per_s"], 1) for nm, v in p.items() if isinstance(v, dict) and "frames_per_s" in v} for k2, p in rnd.items()}), flush=True)
        json.dump(out, open(a.out, "w"), indent=1)


def weld_rows(d, suffix, value):
    """{kernel: value(row)} of the k_weld_* rows of the rocprofv3 CSV `*suffix` under d."""
    f = glob.glob(os.path.join(d, "**", "*" + suffix), recursive=True)
    if not f: raise SystemExit("no %s under %s" % (suffix, d))
    out = collections.OrderedDict()
    for r in csv.DictReader(open(f[0])):
        name = re.sub(r"\(.*", "", r.get("Name") or r.get("Kernel_Name")).replace("void ", "")
        if name.startswith("k_weld"): value(out, name, r)
    return out


def main():
    ap = argparse.ArgumentParser(); ap.add_argument("n", nargs="?", type=int, default=1920); ap.add_argument("--child"); ap.add_argument("--lib")
    ap.add_argument("--parent-lib"); ap.add_argument("--pairs", type=int, default=3); ap.add_argument("--prof-frames", type=int, default=240)
    ap.add_argument("--out"); ap.add_argument("--packed", action="store_true"); ap.add_argument("--dest", default="dev", choices=("dev", "host", "pinned"))
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, "profiles", "r07_packed_points.json" if a.packed else "r08_points_decode.json")
    if a.child == "packed":
        return child_packed(a.n, a.dest, a.lib)
    if a.child:
        return child(a.n, a.child, a.lib)
    if a.packed:
        return main_packed(a)
    out = dict(frames_per_call=a.n, repeats_per_process=REPEATS, pairs=[], note="alternated in fresh processes: this build's uvol_decode_mesh_batch_points "
               "(device outputs) / the parent build's and this build's uvol_decode_mesh_batch_dev; frames_per_s is the best of ms_calls; groups_ms are the "
               "library's event brackets of one further call")
    def one(mode, lib, n=a.n, wrap=()):
        cmd = list(wrap) + [sys.executable, os.path.abspath(__file__), str(n), "--child", mode] + (["--lib", lib] if lib else [])
        env = dict(os.environ, UVOL_WS_DUMP="1")
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
        if r.returncode != 0:
            raise SystemExit("child %s failed (%d): %s" % (mode, r.returncode, r.stderr[-2000:]))       # nothing more is started after a failure
        res = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
        res["workspace_lines"] = sorted(set(l for l in r.stderr.splitlines() if "geometry decode" in l))
        return res
    for k in range(a.pairs):
        pair = dict(points=one("points", None), parent_dev=one("dev", a.parent_lib), this_dev=one("dev", None))
        out["pairs"].append(pair)
        print(json.dumps({k2: {n: round(v["frames_per_s"], 1) for n, v in p.items() if isinstance(v, dict) and "frames_per_s" in v} for k2, p in pair.items()}), flush=True)
        json.dump(out, open(a.out, "w"), indent=1)
    # the weld kernels by the profiler's own clock, then their traffic: one pass each (counters are never collected with anything else)
    nprof = a.prof_frames
    with tempfile.TemporaryDirectory() as td:
        res = one("points", None, nprof, ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", td, "-o", "points", "--"])
        def stat(o, name, r): o[name] = dict(calls=int(r["Calls"]), total_ms=round(float(r["TotalDurationNs"]) / 1e6, 3))
        calls = 2 * (REPEATS + 2)                                           # both layouts, warm-up + REPEATS + one bracketed call each
        out["rocprof_kernel_stats"] = dict(frames_per_call=nprof, decode_calls_in_the_process=calls, kernels=weld_rows(td, "kernel_stats.csv", stat),
                                           weld_group_ms_event_brackets={k: res[k]["groups_ms"].get("geodec.k9_weld") for k in ("interleaved", "planar")},
                                           compulsory_bytes_per_call=res["weld_compulsory_bytes"])
        ks = out["rocprof_kernel_stats"]; ks["weld_ms_per_call"] = round(sum(v["total_ms"] for v in ks["kernels"].values()) / calls, 3)
    json.dump(out, open(a.out, "w"), indent=1)
    traffic = {}
    for counter in ("FETCH_SIZE", "WRITE_SIZE"):
        with tempfile.TemporaryDirectory() as td:
            one("points", None, nprof, ["rocprofv3", "--pmc", counter, "--kernel-trace", "--output-format", "csv", "-d", td, "-o", "points", "--"])
            def add(o, name, r):
                if r["Counter_Name"] == counter: o[name] = o.get(name, 0.0) + float(r["Counter_Value"]) * 1024       # counter unit: KiB
            traffic[counter + "_bytes"] = weld_rows(td, "counter_collection.csv", add)
    ks["counters"] = dict(traffic, note="sums over the process's %d decode calls; profiles/r03_pmc_calibration.json: FETCH_SIZE reads about half of a "
                          "streamed request, WRITE_SIZE the whole" % calls)
    ks["measured_bytes_per_call"] = dict(fetch=sum(traffic["FETCH_SIZE_bytes"].values()) / calls, write=sum(traffic["WRITE_SIZE_bytes"].values()) / calls)
    json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
