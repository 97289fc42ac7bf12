#!/usr/bin/env python3
"""What the device downscale costs: profiled uvol_downscale_rgba_batch_dev calls of N RGBA8 layers of SIZE^2 resident in HBM, factors 2, 4 and 8
(the library's `ingest.downscale` event bracket, uvol_profile_*: input + output bytes are its algorithmic bytes), next to a device-to-device
copy of the same N layers timed in the same run (torch copy_ = hipMemcpyDtoD; read + written bytes) and the achievable HBM rate of
MI355X_MICROARCH.md.  The layers are 16 distinct noise images repeated (noise: every table look-up of a wave goes to a different LDS word).
JSON to stdout.  usage: downscale_timing.py [layers=640] [size=2048] [runs=3]"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "universal-volumetric_amd"))
import torch
import uvol

n = int(sys.argv[1]) if len(sys.argv) > 1 else 640
size = int(sys.argv[2]) if len(sys.argv) > 2 else 2048
runs = int(sys.argv[3]) if len(sys.argv) > 3 else 3
HBM_ACHIEVABLE = 6.3e12
g = torch.Generator(device="cuda"); g.manual_seed(1)
src = torch.empty((n, size, size, 4), dtype=torch.uint8, device="cuda")
for i in range(min(16, n)):
    src[i] = torch.randint(0, 256, (size, size, 4), dtype=torch.uint8, device="cuda", generator=g)
for i in range(16, n):
    src[i] = src[i % 16]
dst = torch.empty_like(src)
torch.cuda.synchronize()
lbytes = size * size * 4
ptrs = [src.data_ptr() + i * lbytes for i in range(n)]
out = dict(layers=n, size=size, layer_bytes=lbytes, hbm_achievable_bytes_per_s=HBM_ACHIEVABLE)
# the copy of the same layers
ms = []
for _ in range(runs + 1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); dst.copy_(src); b.record(); torch.cuda.synchronize(); ms.append(round(a.elapsed_time(b), 3))
cb = 2 * n * lbytes
out["copy_dtod"] = dict(ms=ms[1:], first_ms=ms[0], bytes_read_plus_written=cb, bytes_per_s=cb / (min(ms[1:]) * 1e-3), fraction_of_hbm=cb / (min(ms[1:]) * 1e-3) / HBM_ACHIEVABLE)
cd = uvol.Codec(device=0)
for f in (2, 4, 8):
    cd.downscale_rgba_batch_dev(ptrs, size, size, f)              # the slot's allocation
    cd.profile(True); per = []
    for _ in range(runs):
        cd.profile_reset(); cd.downscale_rgba_batch_dev(ptrs, size, size, f)
        e = [r for r in cd.profile_report() if r["name"] == "ingest.downscale"][0]
        per.append(dict(ms=round(e["total_ms"], 3), algo_bytes=e["algo_bytes"]))
    cd.profile(False)
    best = min(p["ms"] for p in per); ab = per[0]["algo_bytes"]
    out["factor_%d" % f] = dict(calls=per, bytes_per_s=ab / (best * 1e-3), fraction_of_hbm=ab / (best * 1e-3) / HBM_ACHIEVABLE,
                                input_bytes_per_s=n * lbytes / (best * 1e-3), fraction_of_the_copy_rate=(ab / (best * 1e-3)) / out["copy_dtod"]["bytes_per_s"])
cd.close()
print(json.dumps(out))
