"""The batch shared by tests/test_hipemu_aseg.py (host emulation of the kernels) and tests/test_gpu_aseg.py (MI355X): 13 small frames - a
count that is no multiple of 4, 5 or 16 - built around the places where the attribute vertices of seam-touched vertices can go wrong now
that one thread per FACE starts a fan segment at every flagged edge and walks it rightwards (k_aseg) and the sizes of the attribute
tables' id spaces are published with their record tables (k_pack_tabs).  The hand-built frames are grids of 16 x 12 vertices
(330 faces: two blocks, the second one partly filled) whose value ids are drawn per (vertex, label) from a per-corner label array, so a
seam lies wherever two faces label a shared vertex differently:
  0  a texture seam that runs from the border INTO the patch and ends there: the end vertex has a closed fan with one seam edge, its
     segment wraps the whole fan; normals without a seam (slot 0 only)
  1  a normal seam with BOTH ends inside the patch; texture coordinates without a seam (slot 1 only)
  2  three texture charts that meet at one vertex (three seams) and run into the border (seam-touched boundary vertices), four normal
     charts that meet at another vertex (four seams): both slots, different seam sets; the rest of the border stays untouched
  3  one face that is a texture chart of its own (all three edges flagged in slot 0), a dead-end normal seam elsewhere
  4  positions only
  5  a closed torus with texture coordinates and normals per vertex: no seam, no boundary (every flag byte is zero)
  6  synth.grid_mesh(): boundaries and a hole, no interior seam (flag bytes set, nothing to do)
  7  two patches that share ONE position (two closed fans at it, a non-manifold vertex) with a texture seam through one of the fans
  8  frame 2 in scan-like storage order (synth.shuffle_mesh)
  9  synth.torus_mesh(16, 8): wrap seams in the texture coordinates
  10 - 12  seamed spheres of ~300 vertices, each its own tessellation (synth.distinct_meshes, charts=(3, 2))
Every frame must equal oracle.drc_encode byte for byte.

overflow_frame() is the smallest closed mesh of the synth generators whose attribute vertices exceed the default entry capacity
ecap = min(vmax + 6 F + 3, vmax + vmax / 2 + 4096), vmax = the largest value count (geo_ecap): a torus of V = 40 x 20 = 800 positions,
F = 1600, with per-corner texture ids drawn from only 16 values, so that (almost) every edge is a seam and every corner its own segment:
V + 3 F = 5600 ids against ecap = 800 + 400 + 4096 = 5296.  (V + 6 V > 1.5 V + 4096 needs V > 744.)"""
import numpy as np

N_FRAMES = 13
# the LDS walkers on per-corner records (the default of small calls) and the lane-per-walker kernels on ONE record per face, the form of
# the large calls, in which table 1 is table 0 and k_pack_tabs writes the two attribute tables only (5 walkers and 8 streams per wave:
# 13 frames are no multiple of either)
FORMS = {"lds": {}, "face_records": dict(UVOL_SIMT_W="5", UVOL_ENTROPY_W="8")}
RETRY = "re-encoding with worst-case workspace"
NX, NY = 16, 12


def _grid(nx=NX, ny=NY, seed=3, shift=(0.0, 0.0, 0.0)):
    """Open nx x ny patch: positions, faces (two per quad, quad (i, j) -> faces 2 * (j * (nx - 1) + i) and + 1)."""
    rng = np.random.default_rng(seed)
    xs, ys = np.meshgrid(np.arange(nx), np.arange(ny))
    pos = np.stack([xs * 10.0, ys * 10.0, 12.0 * np.sin(xs * 0.5) * np.cos(ys * 0.4)], -1).reshape(-1, 3).astype(np.float32)
    pos += rng.standard_normal(pos.shape).astype(np.float32) * 0.3 + np.array(shift, np.float32)
    f = []
    for j in range(ny - 1):
        for i in range(nx - 1):
            a, b, c, d = j * nx + i, j * nx + i + 1, (j + 1) * nx + i, (j + 1) * nx + i + 1
            f += [(a, b, c), (b, d, c)]
    return pos, np.array(f, np.int64)


def _values(pos, nx=NX, ny=NY):
    """Per-vertex texture coordinates and normals of a patch."""
    uv = (pos[:, :2] / np.array([nx * 10.0, ny * 10.0], np.float32) * 0.5 + 0.05).astype(np.float32)
    n = np.stack([-0.3 * np.cos(pos[:, 0] * 0.05), 0.2 * np.sin(pos[:, 1] * 0.04), np.ones(len(pos))], -1)
    return uv, (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)


def _ids(faces, lab, vals, step):
    """Value ids per (vertex, label): corners of one vertex that carry different labels get different ids (and values `step` apart)."""
    key = (lab.astype(np.int64) << 32) | faces
    uniq, inv = np.unique(key.reshape(-1), return_inverse=True)
    out = vals[uniq & 0xffffffff] + (uniq >> 32)[:, None].astype(np.float32) * np.asarray(step, np.float32)
    return out.astype(np.float32), inv.reshape(-1).astype(np.uint32)


def _quad_of_face(nx=NX, ny=NY):
    q = np.repeat(np.arange((nx - 1) * (ny - 1)), 2)
    return q % (nx - 1), q // (nx - 1)          # column, row of the quad of every face


def _cut_row(faces, j, i0, i1, nx=NX):
    """Labels of a seam along row j: the faces ABOVE the row (quads of row j) label the row's vertices of columns [i0, i1) 1.  The seam
    covers the edges between columns max(i0 - 1, 0) and i1 and ends at both of them where they lie inside the patch."""
    qi, qj = _quad_of_face()
    lab = np.zeros(faces.shape, np.int64)
    on = (faces // nx == j) & (faces % nx >= i0) & (faces % nx < i1)
    lab[on & (qj == j)[:, None]] = 1
    return lab


def _charts(chart_of_face, faces):
    return np.repeat(chart_of_face[:, None], 3, axis=1)


def _mesh(pos, faces, lab_uv=None, lab_nrm=None, uv=None, nrm=None):
    if uv is None:
        uv, nrm = _values(pos)
    z = np.zeros(faces.shape, np.int64)
    u, iu = _ids(faces, z if lab_uv is None else lab_uv, uv, (0.5, 0.25))
    n, inr = _ids(faces, z if lab_nrm is None else lab_nrm, nrm, (0.0, 0.0, 0.0))
    if lab_nrm is not None:                      # distinct normals per label (same direction would still be distinct ids; make the values differ too)
        n = n + (np.arange(len(n)) % 7)[:, None].astype(np.float32) * np.float32(0.01)
        n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    return dict(pos=pos, idx_pos=faces.reshape(-1).astype(np.uint32), uv=u, idx_uv=iu, nrm=n, idx_nrm=inr)


def _bowtie():
    """Two patches, the second one moved away, that share one position: interior vertex (5, 5) of both.  Texture seam through the first
    patch's fan at it (row 5, from the border to column 8)."""
    pa, fa = _grid(seed=4)
    pb, fb = _grid(seed=5, shift=(300.0, 0.0, 40.0))
    va = 5 * NX + 5
    fb2 = fb + len(pa)
    fb2[fb2 == va + len(pa)] = va                                        # (position va + len(pa) stays in the array, unused)
    pos = np.concatenate([pa, pb]); faces = np.concatenate([fa, fb2])
    uva, na = _values(pa); uvb, nb = _values(pb - np.array([300.0, 0.0, 40.0], np.float32))
    uv = np.concatenate([uva, uvb + np.float32(0.45)]); nrm = np.concatenate([na, nb])
    # value ids follow the ORIGINAL vertex of every corner, so the two fans at the shared position keep their own values
    own = np.concatenate([fa, fb + len(pa)])
    lab = np.concatenate([_cut_row(fa, 5, 0, 8), np.zeros(fb.shape, np.int64)])
    u, iu = _ids(own, lab, uv, (0.5, 0.25)); n, inr = _ids(own, np.zeros(own.shape, np.int64), nrm, (0.0, 0.0, 0.0))
    return dict(pos=pos, idx_pos=faces.reshape(-1).astype(np.uint32), uv=u, idx_uv=iu, nrm=n, idx_nrm=inr)


def frames():
    import synth
    pos, faces = _grid()
    qi, qj = _quad_of_face()
    three = np.where(qi < 6, 0, np.where(qj < 5, 1, 2))                  # three charts meet at vertex (6, 5)
    four = (qi >= 9).astype(np.int64) + 2 * (qj >= 7)                    # four charts meet at vertex (9, 7)
    one = np.zeros(len(faces), np.int64); one[2 * (4 * (NX - 1) + 7)] = 1      # a face in the middle, a chart of its own
    f2 = _mesh(pos, faces, _charts(three, faces), _charts(four, faces))
    t = synth.torus_mesh(12, 8)
    out = [_mesh(pos, faces, lab_uv=_cut_row(faces, 6, 0, 9)),
           _mesh(pos, faces, lab_nrm=_cut_row(faces, 4, 3, 11)),
           f2,
           _mesh(pos, faces, _charts(one, faces), _cut_row(faces, 8, 10, NX)),
           dict(pos=pos, idx_pos=faces.reshape(-1).astype(np.uint32)),
           dict(t, uv=np.ascontiguousarray(t["pos"][:, :2] / 300 + 0.5), idx_uv=t["idx_pos"].copy()),
           synth.grid_mesh(),
           _bowtie(),
           synth.shuffle_mesh(f2, seed=11),
           synth.torus_mesh(16, 8)] + synth.distinct_meshes(3, 24, 13, bases=3, charts=(3, 2))
    assert len(out) == N_FRAMES and N_FRAMES % 4 and N_FRAMES % 5 and N_FRAMES % 16
    return out


def seam_census(f, which):
    """(faces with all three edges cut, most seam edges at one vertex, vertices off the border with exactly one seam edge) of attribute `which` ("uv" /
    "nrm") of a manifold frame, from the index arrays alone: what the docstring above promises about the hand-built frames."""
    ip = np.asarray(f["idx_pos"], np.int64).reshape(-1, 3); ia = np.asarray(f["idx_" + which], np.int64).reshape(-1, 3)
    edges = {}
    for fi in range(len(ip)):
        for k in range(3):
            a, b = ip[fi, (k + 1) % 3], ip[fi, (k + 2) % 3]
            edges.setdefault((min(a, b), max(a, b)), []).append((fi, {a: ia[fi, (k + 1) % 3], b: ia[fi, (k + 2) % 3]}))
    cut_per_face = np.zeros(len(ip), int); per_vertex = {}; border = set()
    for (a, b), fs in edges.items():
        if len(fs) == 1:
            cut_per_face[fs[0][0]] += 1; border.update((a, b))
        elif fs[0][1] != fs[1][1]:
            for fi, _ in fs: cut_per_face[fi] += 1
            per_vertex[a] = per_vertex.get(a, 0) + 1; per_vertex[b] = per_vertex.get(b, 0) + 1
    cnt = list(per_vertex.values())
    return int((cut_per_face == 3).sum()), max(cnt, default=0), sum(1 for v, c in per_vertex.items() if c == 1 and v not in border)


def overflow_frame():
    import synth
    t = synth.torus_mesh(40, 20)
    rng = np.random.default_rng(17)
    uv = rng.random((16, 2)).astype(np.float32)
    return dict(t, uv=uv, idx_uv=rng.integers(0, 16, size=len(t["idx_pos"])).astype(np.uint32))


def oracle_bytes(O, f):
    return O.drc_encode(f["pos"], f["idx_pos"], f.get("uv"), f.get("idx_uv"), f.get("nrm"), f.get("idx_nrm"))


_WANT = {}


def want(O):
    """The oracle's bytes of the batch and of the overflow frame, computed once per process."""
    if not _WANT:
        _WANT["batch"] = [oracle_bytes(O, f) for f in frames()]
        _WANT["overflow"] = oracle_bytes(O, overflow_frame())
    return _WANT


def run_batch(O, cd):
    """The 13 frames in one call, then the overflow frame between two good ones: byte for byte the oracle's."""
    fs = frames(); w = want(O)
    got = cd.encode_mesh_batch(fs)
    for i in range(len(fs)):
        assert got[i] == w["batch"][i], "frame %d differs from the oracle" % i
    got = cd.encode_mesh_batch([fs[2], overflow_frame(), fs[0]])
    assert got[0] == w["batch"][2] and got[2] == w["batch"][0], "a neighbour of the overflowing frame differs from the oracle"
    assert got[1] == w["overflow"], "the re-encoded frame differs from the oracle"
