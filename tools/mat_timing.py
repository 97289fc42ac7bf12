#!/usr/bin/env python3
"""What the material attribute costs: one blocking geometry call of N frames resident in HBM (the bench's mesh generator, 100 k vertices,
64 distinct connectivities whose input buffers the frames share) with material 0 on every frame, against the same call without
materials on the same build.  Wall time of alternating runs + the library's per-kernel-group profile (uvol_profile_*).  JSON to stdout.
usage: mat_timing.py [frames=2560] [runs=3] [both|plain|materials]   (one side only: for a kernel trace of that side alone)"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "universal-volumetric_amd"))
import numpy as np
import torch
import uvol, synth

n = int(sys.argv[1]) if len(sys.argv) > 1 else 2560
runs = int(sys.argv[2]) if len(sys.argv) > 2 else 3
mode = sys.argv[3] if len(sys.argv) > 3 else "both"
nd = min(64, n)
base = synth.distinct_meshes(nd, bases=16)
keep, ms, mats = [], [], []
for f in base:
    m, arrs = uvol.Codec._mesh_host(**f)
    dev = [torch.from_numpy(a).cuda() for a in arrs]
    z = torch.zeros(m.n_faces, dtype=torch.uint8, device="cuda")
    keep.append((dev, z))
    m.pos, m.uv, m.nrm, m.idx_pos, m.idx_uv, m.idx_nrm = (t.data_ptr() for t in dev)
    ms.append(m); mats.append(z.data_ptr())
torch.cuda.synchronize()
arr = (uvol.Mesh * n)(*[ms[i % nd] for i in range(n)])
mp = [mats[i % nd] for i in range(n)]
cd = uvol.Codec(device=0, max_batch=n)
plain = lambda: cd.encode_mesh_batch_dev(arr, views=True)
withm = lambda: cd.encode_mesh_batch_dev_mat(arr, mp, views=True)
sides = [(k, f) for k, f in (("plain", plain), ("materials", withm)) if mode in ("both", k)]
out = dict(frames=n, distinct=nd, shared_input_buffers=True)
for k, fn in sides:                                         # warm-up: allocations, both layouts
    out["bytes_per_frame_" + k] = sum(len(r) for r in fn()) / n; out["wall_ms_" + k] = []
for _ in range(runs):
    for k, fn in sides:
        t = time.perf_counter(); fn(); out["wall_ms_" + k].append(round((time.perf_counter() - t) * 1e3, 2))
for k, fn in sides:
    cd.profile(True); cd.profile_reset(); fn()
    out["groups_" + k] = {g["name"]: round(g["total_ms"], 3) for g in cd.profile_report() if g["name"].startswith("geo.")}
    cd.profile(False)
    out["frames_per_s_" + k] = round(n / (min(out["wall_ms_" + k]) / 1e3), 1)
cd.close()
print(json.dumps(out))
