#!/usr/bin/env python3
"""What the mip chain costs (uvol_mipchain_rgba_batch_dev, csrc/tex_mipchain.hip): N RGBA8 layers of SIZE^2 resident in HBM - the workload of
tools/downscale_timing.py, 16 distinct noise images repeated -, in one session:
  * levels 1 - 3 by ONE chain call (the library's `ingest.mipchain` event bracket) against the only way to make them without the chain: three
    uvol_downscale_rgba_batch_dev calls, factors 2, 4, 8 (`ingest.downscale`, summed), with the run-to-run spread of both;
  * the full chain, and its achieved HBM bytes/s against the bytes it must move (level 0 read once plus the levels written: a third);
  * the UASTC encode of tools/uastc_timing.py's workload (2048^2 x 5 layers per segment) with the full chain against one level.
JSON to stdout.  usage: mipchain_timing.py [layers=640] [size=2048] [runs=5] [segments=24]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "universal-volumetric_amd"))
import torch
import uvol

n = int(sys.argv[1]) if len(sys.argv) > 1 else 640
size = int(sys.argv[2]) if len(sys.argv) > 2 else 2048
runs = int(sys.argv[3]) if len(sys.argv) > 3 else 5
nseg = int(sys.argv[4]) if len(sys.argv) > 4 else 24
HBM_ACHIEVABLE = 6.3e12
g = torch.Generator(device="cuda"); g.manual_seed(1)
src = torch.empty((n, size, size, 4), dtype=torch.uint8, device="cuda")
for i in range(min(16, n)):
    src[i] = torch.randint(0, 256, (size, size, 4), dtype=torch.uint8, device="cuda", generator=g)
for i in range(16, n):
    src[i] = src[i % 16]
torch.cuda.synchronize()
lbytes = size * size * 4
ptrs = [src.data_ptr() + i * lbytes for i in range(n)]
out = dict(layers=n, size=size, layer_bytes=lbytes, runs=runs, hbm_achievable_bytes_per_s=HBM_ACHIEVABLE)
cd = uvol.Codec(device=0)


def group(name):
    e = [r for r in cd.profile_report() if r["name"] == name]
    return (sum(r["total_ms"] for r in e), sum(r["algo_bytes"] for r in e))


def stats(ms):
    return dict(ms=[round(x, 3) for x in ms], best_ms=round(min(ms), 3), spread_ms=round(max(ms) - min(ms), 3))


# warm-up: the slots' allocations
for f in (2, 4, 8):
    cd.downscale_rgba_batch_dev(ptrs, size, size, f, slot=f & 1)
cd.mipchain_rgba_batch_dev(ptrs, size, size, 0)
cd.profile(True)
three, chain3, full = [], [], []
for _ in range(runs):                                      # interleaved, so that a drift of the clocks hits both alike
    cd.profile_reset()
    for f in (2, 4, 8):
        cd.downscale_rgba_batch_dev(ptrs, size, size, f, slot=f & 1)
    three.append(group("ingest.downscale")[0])
    cd.profile_reset(); cd.mipchain_rgba_batch_dev(ptrs, size, size, 4)
    chain3.append(group("ingest.mipchain")[0])
    cd.profile_reset(); cd.mipchain_rgba_batch_dev(ptrs, size, size, 0)
    ms, ab = group("ingest.mipchain"); full.append(ms); full_bytes = ab
cd.profile(False)
out["levels_1_to_3_three_downscale_calls"] = stats(three)
out["levels_1_to_3_one_chain_call"] = stats(chain3)
out["chain_over_three_calls"] = round(min(chain3) / min(three), 4)
out["chain_within_the_spread_of_the_three_calls"] = bool(min(chain3) <= min(three) + (max(three) - min(three)))
nl = cd.mip_level_count(size, size)
must = n * lbytes + sum(n * max(1, size >> v) ** 2 * 4 for v in range(1, nl))
out["full_chain"] = dict(levels=nl, **stats(full), bytes_it_must_move=must, algo_bytes=full_bytes, bytes_per_s=must / (min(full) * 1e-3),
                         fraction_of_hbm=must / (min(full) * 1e-3) / HBM_ACHIEVABLE)
cd.close()
del src
torch.cuda.empty_cache()

# the encode: tools/uastc_timing.py's workload, full chain against one level
import synth
B, S = 5, 2048
tex = synth.texture_sequence(B, size=S, seed=0)
dev = [torch.from_numpy(a).cuda() for a in tex]
eptrs = []; keep = []
for s in range(nseg):
    seg = dev if s == 0 else [torch.roll(t, shifts=(4 * s) % S, dims=1).contiguous() for t in dev]
    keep.append(seg); eptrs += [t.data_ptr() for t in seg]
torch.cuda.synchronize()
cu = uvol.Codec(device=0, uastc=1)
enc = {}
for name, levels in (("one_level", 1), ("full_chain", 0)):
    cu.encode_texture_segments_mips(None, levels, dev_ptrs=eptrs, shape=(S, S, B))
    cu.profile(True); wall = []; kern = []
    for _ in range(3):
        cu.profile_reset()
        t = time.perf_counter(); files, st = cu.encode_texture_segments_mips(None, levels, dev_ptrs=eptrs, shape=(S, S, B)); wall.append((time.perf_counter() - t) * 1e3)
        kern.append(sum(r["total_ms"] for r in cu.profile_report() if r["name"] in ("tex.uastc_encode", "tex.uastc_encode_mips", "ingest.mipchain")))
    cu.profile(False)
    assert st == [0] * nseg
    enc[name] = dict(levels=cu.ktx2_levels(files[0]), bytes_per_segment=len(files[0]), wall=stats(wall), kernels=stats(kern))
enc["kernel_ratio_full_over_one"] = round(enc["full_chain"]["kernels"]["best_ms"] / enc["one_level"]["kernels"]["best_ms"], 4)
enc["wall_ratio_full_over_one"] = round(enc["full_chain"]["wall"]["best_ms"] / enc["one_level"]["wall"]["best_ms"], 4)
enc["segments"] = nseg
out["uastc_encode"] = enc
cu.close()
print(json.dumps(out))
