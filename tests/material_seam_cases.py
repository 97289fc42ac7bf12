"""Checks of the material attribute of frames in which materials MEET AT SHARED VERTICES (`uvol_params.material_seams = 1`: the attribute
is written as a Draco MESH_CORNER_ATTRIBUTE), shared by tests/test_hipemu_material_seams.py (host emulation of the kernels) and
tests/test_gpu_material_seams.py (MI355X).

The judge is the repository's oracle DECODER, which is generic over attribute-data slots, plus a face matching that knows nothing of the
encoder: every decoded face is matched to the input face with the nearest centroid; the matching must be injective and every distance
below one quantisation step.  The expected id of a decoded face is its input face's id.

No stock file with an interior material seam is at hand (every recorded file of the reference has one material), so nothing here is a
byte pin against stock draco_encoder: the row is the recorded fourth decoder's with dec_type 1, the seam stream is what the oracle's rabs
coder (pinned to stock) gives for the bits derived from the decoded table, and the values are judged through the decoder.

The library's own decode entry points do not read the corner form yet (include/uvol_codec.h, uvol_decode_mesh_batch_mat), so there is no
check of them here; tests/material_cases.py::run_decoder keeps pinning what they do."""
import ctypes as C
import os
import numpy as np
import material_cases as MC
from material_cases import nfaces, plain, permute_faces


# ---------------------------------------------------------------------------------------------- the matching
def face_centroids(pos, idx):
    p = np.asarray(pos, np.float64).reshape(-1, 3)[np.asarray(idx, np.int64).reshape(-1, 3)]
    return p.mean(1)


def match_faces(m, d):
    """-> input face index per decoded face.  Asserts: injective, every distance below one quantisation step (range / (2^qbits - 1))."""
    p = d.att("position")
    dec = p["float"].astype(np.float64)[p["corner_to_entry"]].reshape(-1, 3, 3).mean(1)
    inp = face_centroids(m["pos"], m["idx_pos"])
    step = p["range"] / ((1 << p["qbits"]) - 1)
    best = np.empty(len(dec), np.int64); dist = np.empty(len(dec))
    for a in range(0, len(dec), 512):                                           # (blocks: a few hundred to ~2000 faces on either side)
        dd = np.linalg.norm(dec[a:a + 512, None, :] - inp[None, :, :], axis=2)
        best[a:a + 512] = dd.argmin(1); dist[a:a + 512] = dd.min(1)
    assert len(np.unique(best)) == len(best), "the face matching is not injective"
    assert dist.max() < step, (dist.max() / step,)
    return best


# ---------------------------------------------------------------------------------------------- id patterns
def torus_halves():
    import synth
    t = synth.torus_mesh(); fm = np.zeros(nfaces(t), np.uint8); fm[nfaces(t) // 2:] = 3
    return t, fm


def _sphere():
    import synth
    return synth.sphere_mesh(40, 21, charts=(5, 4))


def sphere_bands(m=None, bands=4, ids=(0, 1, 2, 3)):
    """Latitude bands (the sphere's polar axis is y): they cross the UV chart seams."""
    m = m or _sphere()
    y = face_centroids(m["pos"], m["idx_pos"])[:, 1]
    k = np.minimum(((y - y.min()) / (np.ptp(y) + 1e-9) * bands).astype(np.int64), bands - 1)
    return m, np.asarray(ids, np.uint8)[k]


def sphere_charts():
    """One id per UV chart: material seams coincide with UV seams."""
    m = _sphere(); cs, cr = 5, 4
    uv = np.asarray(m["uv"], np.float64).reshape(-1, 2)[np.asarray(m["idx_uv"]).reshape(-1, 3)].mean(1)      # (a chart's cell holds all three corners)
    fm = (np.minimum((uv[:, 1] * cr).astype(np.int64), cr - 1) * cs + np.minimum((uv[:, 0] * cs).astype(np.int64), cs - 1)).astype(np.uint8)
    assert len(set(fm.tolist())) == cs * cr
    return m, fm


def grid_stripes():
    """Vertical stripes: the seams end on the mesh boundary and at the hole."""
    import synth
    g = synth.grid_mesh()
    x = face_centroids(g["pos"], g["idx_pos"])[:, 0]
    return g, ((x // 30.0).astype(np.int64) % 3 + 1).astype(np.uint8)


def grid_checkerboard(nx=24, ny=16):
    """Every face its neighbours' opposite: every interior edge is a seam, 3 attribute vertices per face.  The compact workspace holds
    1.5 x the largest input attribute + 4096 entries, so the 40 x 28 grid (2074 faces, 1120 vertices: 7342 attribute vertices against 5776)
    takes the GEO_E_WS_OVERFLOW retry - alone, with worst-case sizes -, the default grid does not."""
    import synth
    g = synth.grid_mesh(nx, ny); nf = nfaces(g)
    idx = np.asarray(g["idx_pos"]).reshape(-1, 3)
    # two-colour the dual graph (a planar triangulated lattice: faces across an edge alternate)
    edges = {}
    for f in range(nf):
        for k in range(3):
            e = tuple(sorted((int(idx[f, k]), int(idx[f, (k + 1) % 3])))); edges.setdefault(e, []).append(f)
    adj = [[] for _ in range(nf)]
    for fs in edges.values():
        if len(fs) == 2: adj[fs[0]].append(fs[1]); adj[fs[1]].append(fs[0])
    col = np.full(nf, -1, np.int64)
    for s in range(nf):
        if col[s] >= 0: continue
        col[s] = 0; todo = [s]
        while todo:
            a = todo.pop()
            for b in adj[a]:
                if col[b] < 0: col[b] = 1 - col[a]; todo.append(b)
    assert all(col[a] != col[b] for a in range(nf) for b in adj[a])
    return g, np.where(col == 0, 4, 9).astype(np.uint8)


def sphere_pinwheel():
    """Five ids around the top pole (one vertex, 40 faces in its fan), a sixth on the rest."""
    m = _sphere(); fm = np.full(nfaces(m), 6, np.uint8)
    fm[:40] = (np.arange(40) // 8 + 1).astype(np.uint8)                         # (the top cap is stored first)
    return m, fm


def torus_island():
    """A single-face island."""
    import synth
    t = synth.torus_mesh(); fm = np.full(nfaces(t), 2, np.uint8); fm[777] = 200
    return t, fm


def torus_0_255():
    import synth
    t = synth.torus_mesh(); fm = np.zeros(nfaces(t), np.uint8); fm[1::2] = 255
    return t, fm


def small_sphere_bands():
    import synth
    return sphere_bands(synth.sphere_mesh(16, 9, charts=(2, 2)), bands=3, ids=(7, 0, 255))


def shells_split(degenerate=False):
    """The five-shell frame of material_cases with its second shell (the sphere) split in two by height; optionally behind the degenerate
    first face of material_cases.degenerate_frame()."""
    if degenerate: m, fm, spans, ids = MC.degenerate_frame()
    else: name, m, fm, spans, ids = MC.value_frames()[2]
    fm = np.array(fm, np.uint8)
    y = face_centroids(m["pos"], m["idx_pos"])[:, 1]
    sel = fm == 7
    first = np.flatnonzero(sel)[0]
    while not sel[first:first + 1600].all(): first += 1                         # (the first shell with id 7 is the torus; the sphere has 1600 faces)
    sph = np.zeros(len(fm), bool); sph[first:first + 1600] = True
    fm[sph & (y > np.median(y[sph]))] = 77
    return m, fm


def soup():
    import synth
    m = synth.random_soup_mesh(2)
    return m, np.random.default_rng(23).integers(0, 5, nfaces(m)).astype(np.uint8)


def seam_frames():
    """(name, mesh, ids, dropped faces)."""
    out = [("torus_halves",) + torus_halves() + (0,), ("sphere_bands",) + sphere_bands() + (0,), ("sphere_charts",) + sphere_charts() + (0,),
           ("grid_stripes",) + grid_stripes() + (0,), ("sphere_pinwheel",) + sphere_pinwheel() + (0,), ("torus_island",) + torus_island() + (0,),
           ("grid_checkerboard",) + grid_checkerboard() + (0,), ("grid_checkerboard_retry",) + grid_checkerboard(40, 28) + (0,), ("torus_0_255",) + torus_0_255() + (0,), ("small_sphere_bands",) + small_sphere_bands() + (0,),
           ("shells_split",) + shells_split() + (0,), ("shells_split_degenerate",) + shells_split(True) + (1,), ("soup",) + soup() + (None,)]
    return out


def shuffled(frames, seed=31):
    out = []
    for k, (name, m, fm, dropped) in enumerate(frames):
        ms, fms = permute_faces(m, fm, seed + k)
        out.append((name + "_shuffled", ms, fms, dropped))
    return out


# ---------------------------------------------------------------------------------------------- checks on one stream
def expected_bits(d, ids):
    """Seam bits in the decoder's order (oracle/drc_dec.c, "seams"): faces ascending, corners 0..2, boundary corners and edges whose other
    face has the lower index skipped; 1 when the ids of the two faces differ.  -> (bits, boundary corners, seam edges)."""
    opp = d.opp; bits = []; nb = 0
    for c in range(3 * d.nf):
        o = int(opp[c])
        if o < 0: nb += 1; continue
        if o // 3 < c // 3: continue
        bits.append(1 if ids[c // 3] != ids[o // 3] else 0)
    bits = np.array(bits, np.uint8)
    return bits, nb, int(bits.sum())


def corner_classes(d, ids):
    """Number of attribute vertices the decoder must find: corner classes under 'same vertex, adjacent across an interior non-seam edge'
    (union-find over the decoded table; it does not restate the encoder)."""
    n = 3 * d.nf; par = list(range(n))
    def find(a):
        while par[a] != a: par[a] = par[par[a]]; a = par[a]
        return a
    nxt = lambda c: c - 2 if c % 3 == 2 else c + 1
    prv = lambda c: c + 2 if c % 3 == 0 else c - 1
    for c in range(n):
        o = int(d.opp[c])
        if o < 0 or ids[c // 3] != ids[o // 3]: continue
        for a, b in ((nxt(c), prv(o)), (prv(c), nxt(o))):
            ra, rb = find(a), find(b)
            if ra != rb: par[ra] = rb
    return len({find(c) for c in range(n)})


def check_stream(O, cd, name, m, fm, dropped, data, base, pin):
    """Checks 1 - 5 on one stream written with material_seams = 1 (base: the same frame without materials)."""
    row, sec = pin
    d = O.drc_decode(data)
    nad = len(d.atts) - 1
    # 1: nothing left over; the recorded fourth decoder's row with dec_type 1 (att_data_id and unique_id follow nad as in check_stock_row)
    assert d.leftover == 0 and d.nad == nad, name
    a = d.atts[nad]
    want_row = dict(row, unique_id=nad, att_data_id=nad - 1, dec_type=1)
    assert {k: a[k] for k in MC.ROW_FIELDS} == want_row, (name, {k: a[k] for k in MC.ROW_FIELDS})
    # 2: connectivity, every other attribute's values, maps and section bytes are those of the stream without materials
    MC.check_against_plain(O, data, base)
    # expected ids through the matching
    src = match_faces(m, d)
    want = np.asarray(fm)[src]
    if dropped is not None: assert d.nf == nfaces(m) - dropped, (name, d.nf)
    else: assert d.nf <= nfaces(m)
    # 3: the material slot's seam stream
    bits, nb, ns = expected_bits(d, want)
    assert ns > 0, name                                                         # (the frame does have an interior material seam)
    pieces = MC.seam_pieces(data)
    assert len(pieces) == 1 + d.nad and pieces[-1] == O.rabs_encode(bits), (name, len(bits), pieces[-1][:8].hex())
    # 4: counts.  n_seam_corners is the oracle's count of seam marks: one per boundary corner and one per interior seam EDGE (drc_dec.c flags
    # the edge's two corners together and counts them once), i.e. the flagged corners - boundary corners + 2 x seam edges - less one per
    # seam edge.  Both forms are asserted, from counts taken on the decoded table.
    flagged = nb + 2 * ns
    assert a["n_seam_corners"] == flagged - ns == nb + ns, (name, a["n_seam_corners"], nb, ns)
    assert a["n"] == corner_classes(d, want), (name, a["n"])
    # 5: values: one id on the three corners of every face, the expected one; the length within the bound
    fv = MC.face_values(d)
    assert np.array_equal(fv[:, 0], fv[:, 1]) and np.array_equal(fv[:, 0], fv[:, 2]), name
    assert np.array_equal(fv[:, 0], want), (name, int((fv[:, 0] != want).sum()))
    mh, keep = cd._mesh_host(**plain(m))
    # Why 8 bytes per face (uvol_mesh_bound_mat = uvol_mesh_bound + 4096 + 8 * faces) covers the corner form's worst case, the checkerboard:
    # it codes at most 3 symbols per face (one attribute vertex per corner).  A symbol is below 512 (wrap-corrected residuals of 8-bit
    # values), so its rANS table is below 3 * 512 bytes (inside the 4096) and the payload, coded with frequencies proportional to the counts,
    # stays below log2(512) = 9 bits + rounding per symbol: < 1.25 bytes, 3.75 per face.  The seam stream holds at most 1.5 bits per face
    # (one per interior edge) and the rabs coder spends at most ~1 bit per bit at its 8-bit probability: < 0.25 bytes per face.  4 < 8.
    assert len(data) <= cd.L.uvol_mesh_bound_mat(C.byref(mh)), name
    return d


def run_streams(O, cd_seams, frames):
    """Checks 1 - 5 for every frame, encoded in one batch; -> the streams."""
    pin = MC.stock_pin(O)
    res = cd_seams.encode_mesh_batch([dict(m, face_mat=fm) for _, m, fm, _ in frames])
    base = cd_seams.encode_mesh_batch([plain(m) for _, m, _, _ in frames])
    for (name, m, fm, dropped), r, b in zip(frames, res, base):
        check_stream(O, cd_seams, name, m, fm, dropped, r, b, pin)
    return res


def run_unchanged_without_seams(O, cd_seams, cd_default):
    """Check 6: frames without an interior material seam - zeros, the value frames, no ids - give the default codec's bytes."""
    zeros = [dict(m, face_mat=np.zeros(nfaces(m), np.uint8)) for m in MC.small_meshes()]
    vals = [dict(m, face_mat=fm) for _, m, fm, _, _ in MC.value_frames()]
    bare = [plain(m) for m in MC.small_meshes()]
    for frames in (zeros, vals, bare, zeros[:1] + bare[:1] + vals[2:]):
        assert cd_seams.encode_mesh_batch(frames) == cd_default.encode_mesh_batch(frames)


def run_default_refuses(O, cd_seams, cd_default):
    """Check 7: the two settings side by side on the torus-halves frame."""
    import uvol
    t, fm = torus_halves()
    res = cd_default.encode_mesh_batch([dict(t, face_mat=fm)], raise_on_error=False)
    assert res[0] is None and "material" in cd_default.error()
    r = cd_seams.encode_mesh_batch([dict(t, face_mat=fm)])[0]
    assert O.drc_decode(r).atts[-1]["dec_type"] == 1


def run_ragged(O, cd, mem):
    """Check 8: seamed, seamless-material, no-material, no-uv and no-normal frames in one batch; every frame's bytes are its bytes alone;
    host inputs == device inputs; the enqueue form == the blocking form."""
    import uvol
    t, fm_t = torus_halves(); s, fm_s = sphere_bands(); g, fm_g = grid_stripes()
    no_uv = dict(pos=s["pos"], idx_pos=s["idx_pos"], nrm=s["nrm"], idx_nrm=s["idx_nrm"])
    no_nrm = dict(pos=g["pos"], idx_pos=g["idx_pos"], uv=g["uv"], idx_uv=g["idx_uv"])
    bare = dict(pos=t["pos"], idx_pos=t["idx_pos"])
    frames = [dict(t, face_mat=fm_t), dict(s, face_mat=np.full(nfaces(s), 9, np.uint8)), plain(g), dict(no_uv, face_mat=fm_s), dict(no_nrm, face_mat=fm_g),
              dict(bare, face_mat=fm_t), no_nrm, dict(g, face_mat=grid_checkerboard()[1])]
    res = cd.encode_mesh_batch(frames)
    alone = [cd.encode_mesh_batch([f])[0] for f in frames]
    assert res == alone
    pin = MC.stock_pin(O)
    for i in (0, 3, 4, 5, 7):
        f = frames[i]
        check_stream(O, cd, "ragged %d" % i, f, f["face_mat"], 0, res[i], cd.encode_mesh_batch([plain(f)])[0], pin)
    # device inputs and the enqueue form through the C ABI
    n = len(frames); meshes = (uvol.Mesh * n)(); dmeshes = (uvol.Mesh * n)(); keep = []; fms = []; dfm = (C.c_void_p * n)()
    for i, f in enumerate(frames):
        m, k, fm = cd._mesh_host_mat(**f); meshes[i] = m; keep.append(k); fms.append(fm)
        pos, uv, nrm, ip, iu, inn = k
        dm = uvol.Mesh(); dm.n_pos, dm.n_uv, dm.n_nrm, dm.n_faces = m.n_pos, m.n_uv, m.n_nrm, m.n_faces
        dm.pos = mem.to_dev(pos); dm.idx_pos = mem.to_dev(ip)
        if m.uv: dm.uv = mem.to_dev(uv); dm.idx_uv = mem.to_dev(iu)
        if m.nrm: dm.nrm = mem.to_dev(nrm); dm.idx_nrm = mem.to_dev(inn)
        dmeshes[i] = dm
        dfm[i] = mem.to_dev(fm) if fm is not None else None
    mats = cd._mat_ptrs(fms)
    def call(fn, ms, mp, on_dev, sync):
        outs = (C.c_void_p * n)(); caps = (C.c_size_t * n)(); lens = (C.c_size_t * n)(); st = (C.c_int * n)(); bufs = []
        for i in range(n):
            caps[i] = cd.L.uvol_mesh_bound_mat(C.byref(meshes[i])); bufs.append(np.empty(caps[i], np.uint8)); outs[i] = bufs[i].ctypes.data
        assert fn(cd.h, ms, mp, n, on_dev, outs, caps, lens, st) == 0, cd.error()
        if sync: assert cd.L.uvol_sync(cd.h) == 0, cd.error()
        assert list(st) == [0] * n, list(st)
        return [bufs[i][:lens[i]].tobytes() for i in range(n)]
    assert call(cd.L.uvol_encode_mesh_batch_mat, meshes, mats, 0, False) == res
    assert call(cd.L.uvol_encode_mesh_batch_mat, dmeshes, dfm, 1, False) == res
    assert call(cd.L.uvol_encode_mesh_batch_mat_async, meshes, mats, 0, True) == res
    assert call(cd.L.uvol_encode_mesh_batch_mat_async, dmeshes, dfm, 1, True) == res
    mem.free_all()


def forms_digest(O, cd):
    """The streams of the seamed frames and their shuffled forms, for the fresh-process comparison (check 9)."""
    import hashlib
    F = {f[0]: f for f in seam_frames()}
    frames = [F[k] for k in ("torus_halves", "sphere_bands", "grid_stripes", "sphere_pinwheel", "grid_checkerboard_retry", "soup")]
    frames += shuffled(frames[:2])
    res = run_streams(O, cd, frames)
    return hashlib.sha256(b"".join(res)).hexdigest()
