#!/usr/bin/env python3
"""What the direct ETC2 RGB encode costs and buys: profiled uvol_encode_etc2_rgb_batch calls of N RGBA8 layers of SIZE^2 resident in HBM (the
library's `etc2.encode` event bracket, uvol_profile_*; every layer's blocks are compared with those of the layer it repeats, so all rounds
of the kernel's grid-stride loop are checked at this size), next
to the way the raw `etc2` target was made before it - the ETC1S segment encode of the same layers and uvol_transcode_texture_segments_etc1
of those segments, timed separately (wall clock around the blocking calls, and the transcode's own event brackets) - and a device-to-device
copy of the input bytes as the rate yardstick (torch copy_ = hipMemcpyDtoD).  The layers are the bench's texture (synth.texture_sequence(5,
size, seed=0), bench.py) repeated; the RGB PSNR of both targets against the source is computed on its five layers with the independent
decoder of tests/helpers.py.  JSON to stdout.  usage: etc2_direct_timing.py [layers=640] [size=2048] [runs=3]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "universal-volumetric_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import uvol, synth, helpers

n = int(sys.argv[1]) if len(sys.argv) > 1 else 640
size = int(sys.argv[2]) if len(sys.argv) > 2 else 2048
runs = int(sys.argv[3]) if len(sys.argv) > 3 else 3
B = 5
n -= n % B
tex = synth.texture_sequence(B, size=size, seed=0)
src = torch.empty((n, size, size, 4), dtype=torch.uint8, device="cuda")
for i in range(B):
    src[i] = torch.from_numpy(np.ascontiguousarray(tex[i])).cuda()
for i in range(B, n):
    src[i] = src[i % B]
dst = torch.empty_like(src)
torch.cuda.synchronize()
lbytes = size * size * 4; nbk = (size // 4) ** 2; obytes = nbk * 8
ptrs = [src.data_ptr() + i * lbytes for i in range(n)]
out = dict(layers=n, size=size, layer_bytes=lbytes, blocks=n * nbk, texture="synth.texture_sequence(5, size, seed=0), repeated")
ms = []
for _ in range(runs + 1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); dst.copy_(src); b.record(); torch.cuda.synchronize(); ms.append(round(a.elapsed_time(b), 3))
out["copy_dtod_of_the_input"] = dict(ms=ms[1:], first_ms=ms[0], input_bytes=n * lbytes, input_bytes_per_s=n * lbytes / (min(ms[1:]) * 1e-3))
del dst
blocks = torch.empty((n, obytes), dtype=torch.uint8, device="cuda")
optrs = [blocks.data_ptr() + i * obytes for i in range(n)]
cd = uvol.Codec(device=0)


def psnr(blk, img):
    dec = helpers.etc1_decode_blocks(blk, size, size)[..., :3].astype(np.float64)
    return float(10 * np.log10(255.0 ** 2 / ((dec - img[::-1, :, :3].astype(np.float64)) ** 2).mean()))      # (y_flip = 1: the bottom row is stored first)


cd.encode_etc2_rgb_batch(ptrs, size, size, out_dev_ptrs=optrs)              # warm-up: allocations, code object
cd.profile(True); per = []
for _ in range(runs):
    cd.profile_reset(); cd.encode_etc2_rgb_batch(ptrs, size, size, out_dev_ptrs=optrs)
    e = [r for r in cd.profile_report() if r["name"] == "etc2.encode"][0]
    per.append(round(e["total_ms"], 3))
cd.profile(False)
best = min(per)
direct = blocks[:B].cpu().numpy().reshape(B, size // 4, size // 4, 8)
repeats_agree = all(bool(torch.equal(blocks[i], blocks[i % B])) for i in range(B, n))
out["direct"] = dict(ms_per_launch=per, blocks_per_s=n * nbk / (best * 1e-3), input_bytes_per_s=n * lbytes / (best * 1e-3),
                     fraction_of_the_copy_rate=(n * lbytes / (best * 1e-3)) / out["copy_dtod_of_the_input"]["input_bytes_per_s"],
                     every_layer_equals_the_layer_it_repeats=repeats_agree)
# the parent's way: ETC1S segments, then the re-pack
wall = []
for _ in range(runs + 1):
    t0 = time.perf_counter(); segs = cd.encode_texture_segments_dev(ptrs, B, size, size); wall.append(round((time.perf_counter() - t0) * 1e3, 3))
out["etc1s_segment_encode"] = dict(segments=n // B, wall_ms=wall[1:], first_wall_ms=wall[0], segment_bytes=len(segs[0]))
wall = []; groups = None
for r in range(runs + 1):
    cd.profile(True); cd.profile_reset()
    t0 = time.perf_counter(); tr = cd.transcode_texture_segments_etc1(segs); wall.append(round((time.perf_counter() - t0) * 1e3, 3))
    groups = {e["name"]: round(e["total_ms"], 3) for e in cd.profile_report() if e["name"].startswith("texdec.")}
    cd.profile(False)
out["transcode_segments_etc1"] = dict(wall_ms_host_outputs=wall[1:], first_wall_ms=wall[0], device_ms_by_group_last_run=groups)
out["psnr_rgb_db"] = dict(direct=[round(psnr(direct[l], tex[l]), 3) for l in range(B)], transcoded_from_etc1s=[round(psnr(tr[0][l], tex[l]), 3) for l in range(B)])
cd.close()
print(json.dumps(out))
