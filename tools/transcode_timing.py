#!/usr/bin/env python3
"""Per-target kernel times of the texture transcodes and block encoders on a real GPU, from the library's own profile brackets: every
ETC1S target (`texdec.k3_unpack`, one call per target: an opaque file takes all six, a file with alpha slices the four that accept it),
every UASTC target (`texdec.uastc_*`; etc2_rgba and bc3 also on blocks that carry alpha), `tex.uastc_encode` and `etc2.encode`.  Layers
of SIZE^2, 5 per segment, device outputs; every shape is run once before it is timed.  UVOL_LIB selects another build of the library
(uvol.load), so two builds can be timed in alternating fresh processes.  One JSON line: {bracket:target[:source]: ms}.
usage: tools/transcode_timing.py [etc1s_segments=48] [uastc_segments=24] [size=2048]"""
import ctypes as C, json, os, sys
import torch
torch.zeros(1, device="cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "universal-volumetric_amd"))
import numpy as np
import uvol, synth
nseg_e = int(sys.argv[1]) if len(sys.argv) > 1 else 48
nseg_u = int(sys.argv[2]) if len(sys.argv) > 2 else 24
size = int(sys.argv[3]) if len(sys.argv) > 3 else 2048
B = 5
nbk = (size // 4) ** 2
tex = synth.texture_sequence(B, size=size, seed=3)
texa = [a.copy() for a in tex]
for a in texa:                                                          # alpha: a ramp across the image times the red channel's top bits
    a[..., 3] = (np.arange(size, dtype=np.uint32)[None, :] * 255 // (size - 1)).astype(np.uint8) & (a[..., 0] | 0x1f)
out_buf = torch.empty(max(nseg_e, nseg_u) * B * size * size * 4, dtype=torch.uint8, device="cuda:0")
res = {}


def bracket(cd, name):
    return round(sum(g["total_ms"] for g in cd.profile_report() if g["name"] == name), 3)


def transcode(cd, files, target, name, key):
    code, unit, blocks = cd.TARGETS[target]; n = len(files)
    cap = nbk * unit if blocks else size * size * 4
    fp = (C.c_char_p * n)(*files); ln = (C.c_size_t * n)(*[len(f) for f in files]); st = (C.c_int * n)()
    ptrs = (C.c_void_p * (n * B))(*[out_buf.data_ptr() + i * cap for i in range(n * B)])
    for timed in (False, True):
        cd.profile_reset()
        rc = cd.L.uvol_transcode_texture_segments_st(cd.h, fp, ln, n, ptrs, cap, 1, code, st)
        assert rc == 0 and not any(st), (key, rc, list(st), cd.error())
    res[key] = bracket(cd, name)


cd = uvol.Codec(device=0); cd.profile(True)
for src, layers, targets in (("opaque", tex, ("rgba32", "etc1", "bc7", "etc2_rgba", "bc1", "bc3")), ("alpha", texa, ("rgba32", "bc7", "etc2_rgba", "bc3"))):
    files = [cd.encode_texture_segment(layers)] * nseg_e
    for t in targets:
        transcode(cd, files, t, "texdec.k3_unpack", "texdec.k3_unpack:%s:%s" % (t, src))
# the direct ETC2 encode of the same layers, resident in HBM
dev = torch.stack([torch.from_numpy(np.ascontiguousarray(a)) for a in tex]).cuda()
lptrs = [dev[i % B].data_ptr() for i in range(nseg_e * B)]
optrs = [out_buf.data_ptr() + i * nbk * 8 for i in range(nseg_e * B)]
for timed in (False, True):
    cd.profile_reset(); cd.encode_etc2_rgb_batch(lptrs, size, size, out_dev_ptrs=optrs)
res["etc2.encode"] = bracket(cd, "etc2.encode")
cd.close()

cu = uvol.Codec(device=0, uastc=1); cu.profile(True)
UNAMES = {"rgba32": "texdec.uastc_rgba", "astc": "texdec.uastc_astc", "bc7": "texdec.uastc_bc7", "bc1": "texdec.uastc_bc13", "bc3": "texdec.uastc_bc13",
          "etc1": "texdec.uastc_etc", "etc2_rgba": "texdec.uastc_etc"}
for src, layers, targets in (("opaque", tex, tuple(UNAMES)), ("alpha", texa, ("bc3", "etc2_rgba"))):
    d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in layers]
    keep = [d if s == 0 else [torch.roll(t, shifts=(4 * s) % size, dims=1).contiguous() for t in d] for s in range(nseg_u)]
    ptrs = [t.data_ptr() for seg in keep for t in seg]
    torch.cuda.synchronize()
    for timed in (False, True):
        cu.profile_reset(); files = cu.encode_texture_segments_dev(ptrs, B, size, size)
    res["tex.uastc_encode:%s" % src] = bracket(cu, "tex.uastc_encode")
    del keep
    for t in targets:
        transcode(cu, files, t, UNAMES[t], "%s:%s:%s" % (UNAMES[t], t, src))
cu.close()
print(json.dumps(dict(etc1s_segments=nseg_e, uastc_segments=nseg_u, layers=B, size=size, lib=os.environ.get("UVOL_LIB", "default"), ms=res)))
