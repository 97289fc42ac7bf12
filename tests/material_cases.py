"""Checks of the OBJ material attribute (Draco GENERIC uint8, `usemtl`) shared by tests/test_hipemu_material.py (host emulation of the
kernels) and tests/test_gpu_material.py (MI355X).  Every check takes the oracle module, a uvol.Codec and a Mem: how the caller reaches
"device" memory (the emulation's device memory is host memory; on the GPU it is hipMalloc / hipMemcpy through ctypes).

The judge is the repository's oracle DECODER, which reads the fourth attribute of the reference's recorded files generically; the stock
bytes are read from the fixture files at run time, nothing is typed in."""
import ctypes as C
import os
import numpy as np
from conftest import GOLDEN, ROOT

ROW_FIELDS = ("att_type", "data_type", "ncomp", "unique_id", "dec_type", "att_data_id", "seq_type", "pred_method", "transform")


class HostMem:
    """Device memory of the emulation build = host memory."""
    def __init__(self):
        self.keep = []

    def to_dev(self, a):
        a = np.ascontiguousarray(a); self.keep.append(a); return a.ctypes.data

    def alloc(self, nbytes):
        a = np.zeros(max(16, nbytes), np.uint8); self.keep.append(a); return a.ctypes.data

    def to_host(self, ptr, dtype, count):
        n = count * np.dtype(dtype).itemsize
        return np.frombuffer((C.c_uint8 * n).from_address(ptr), dtype=dtype, count=count).copy() if count else np.zeros(0, dtype)

    def free_all(self):
        self.keep = []


class HipMem:
    """HBM through the HIP runtime (the caller need not be torch)."""
    def __init__(self):
        self.hip = C.CDLL("libamdhip64.so"); self.owned = []

    def alloc(self, nbytes):
        p = C.c_void_p(); assert self.hip.hipMalloc(C.byref(p), C.c_size_t(max(nbytes, 16))) == 0; self.owned.append(p.value); return p.value

    def to_dev(self, a):
        a = np.ascontiguousarray(a); p = self.alloc(a.nbytes)
        if a.nbytes: assert self.hip.hipMemcpy(C.c_void_p(p), C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), C.c_int(1)) == 0
        return p

    def to_host(self, ptr, dtype, count):
        a = np.empty(count, dtype)
        if count: assert self.hip.hipMemcpy(C.c_void_p(a.ctypes.data), C.c_void_p(ptr), C.c_size_t(a.nbytes), C.c_int(2)) == 0
        return a

    def free_all(self):
        for p in self.owned: self.hip.hipFree(C.c_void_p(p))
        self.owned = []


# ---------------------------------------------------------------------------------------------- fixtures and meshes
def stock_pin(O):
    """(row, section bytes) of the fourth decoder of the reference's recorded files, read from the fixtures; both files must agree."""
    got = []
    for name in ("00000.drc", "00075.drc"):
        b = open(os.path.join(GOLDEN, name), "rb").read()
        d = O.drc_decode(b)
        assert d.leftover == 0 and len(d.atts) == 4 and d.nad == 3
        a = d.atts[3]
        assert a["n"] == d.nev
        got.append(({k: a[k] for k in ROW_FIELDS}, b[a["sec_begin"]:a["sec_end"]]))
    assert got[0] == got[1] and len(got[0][1]) == 18
    assert got[0][0] == dict(att_type=4, data_type=2, ncomp=1, unique_id=3, dec_type=0, att_data_id=2, seq_type=1, pred_method=1, transform=1)   # (the issue's table, as a cross-check of the reading)
    return got[0]


def small_meshes():
    import synth
    return [synth.torus_mesh(), synth.sphere_mesh(40, 21, charts=(5, 4)), synth.grid_mesh()]


def nfaces(m):
    return len(m["idx_pos"]) // 3


def shells(parts, ids):
    """Disjoint shells side by side along x (shell k moved so that its x range starts at k * dx, dx = twice the widest shell), shell k
    with material ids[k] on every face.  -> (mesh, face_mat, x intervals per shell)."""
    out = {k: [] for k in ("pos", "uv", "nrm", "idx_pos", "idx_uv", "idx_nrm")}; fm = []; off = dict(pos=0, uv=0, nrm=0); spans = []
    dx = 2.0 * max(float(np.ptp(np.asarray(m["pos"], np.float32).reshape(-1, 3)[:, 0])) for m in parts) + 1.0
    for k, (m, mid) in enumerate(zip(parts, ids)):
        p = np.array(m["pos"], np.float32).reshape(-1, 3).copy(); p[:, 0] += np.float32(k * dx) - p[:, 0].min()
        spans.append((float(p[:, 0].min()), float(p[:, 0].max())))
        out["pos"].append(p); out["uv"].append(np.array(m["uv"], np.float32).reshape(-1, 2)); out["nrm"].append(np.array(m["nrm"], np.float32).reshape(-1, 3))
        for a, w in (("pos", 3), ("uv", 2), ("nrm", 3)):
            out["idx_" + a].append(np.array(m["idx_" + a], np.uint32).reshape(-1) + np.uint32(off[a])); off[a] += len(np.array(m[a]).reshape(-1, w))
        fm += [mid] * nfaces(m)
    return {k: np.concatenate(v) for k, v in out.items()}, np.array(fm, np.uint8), spans


def permute_faces(m, fm, seed):
    """The same mesh with its faces stored in a seeded random order (the ids move with them)."""
    perm = np.random.default_rng(seed).permutation(nfaces(m))
    out = dict(m)
    for k in ("idx_pos", "idx_uv", "idx_nrm"):
        if m.get(k) is not None:
            out[k] = np.array(m[k]).reshape(-1, 3)[perm].reshape(-1)
    return out, np.asarray(fm)[perm]


def value_frames():
    """(name, mesh, face_mat, spans, ids): a single non-zero id, ids 0 and 255, five shells."""
    import synth
    t, s, g, s2 = synth.torus_mesh(), synth.sphere_mesh(40, 21, charts=(5, 4)), synth.grid_mesh(), synth.sphere_mesh(24, 13, charts=(3, 2), crease=False)
    out = []
    for name, parts, ids in (("one_id", [t], [5]), ("0_and_255", [s, t], [0, 255]), ("five_shells", [t, s, g, s2, t], [0, 7, 200, 31, 7])):
        m, fm, spans = shells(parts, ids)
        out.append((name, m, fm, spans, ids))
    return out


def plain(m):
    return {k: m.get(k) for k in ("pos", "idx_pos", "uv", "idx_uv", "nrm", "idx_nrm")}


# ---------------------------------------------------------------------------------------------- checks on one stream
def check_stock_row(O, data, pin, nad=3):
    """Check 1: four decoders, the fixture's row field for field, the fixture's 18 bytes."""
    row, sec = pin
    d = O.drc_decode(data)
    assert d.leftover == 0 and len(d.atts) == nad + 1 and d.nad == nad
    a = d.atts[nad]
    want = dict(row, unique_id=nad, att_data_id=nad - 1)           # (nad == 3: exactly the fixture's row)
    assert {k: a[k] for k in ROW_FIELDS} == want and a["n"] == d.nev, ({k: a[k] for k in ROW_FIELDS}, a["n"], d.nev)
    return d, a


def check_against_plain(O, with_mat, without):
    """Check 2: everything but the material attribute is what the material-less stream holds."""
    d, p = O.drc_decode(with_mat), O.drc_decode(without)
    assert d.leftover == 0 and p.leftover == 0 and len(d.atts) == len(p.atts) + 1 and d.nad == p.nad + 1
    assert np.array_equal(d.opp, p.opp) and np.array_equal(d.c2v, p.c2v)
    for k in range(len(p.atts)):
        a, b = d.atts[k], p.atts[k]
        assert np.array_equal(a["vals"], b["vals"]) and np.array_equal(a["corner_to_entry"], b["corner_to_entry"]), k
        assert with_mat[a["sec_begin"]:a["sec_end"]] == without[b["sec_begin"]:b["sec_end"]], k
    return d


def seam_pieces(data):
    """The rabs sections behind the connectivity header of an edgebreaker stream: start faces, then one seam stream per
    attribute data, each as its bytes (probability byte, varint length, payload)."""
    o = 12                                                                      # "DRACO", version, type, method, flags; the traversal byte
    def varint():
        nonlocal o
        v = s = 0
        while True:
            c = data[o]; o += 1; v |= (c & 0x7f) << s; s += 7
            if c < 0x80: return v
    varint(); varint(); nad = data[o]; o += 1; varint(); varint(); nev = varint()
    for _ in range(2 * nev): varint()
    o += (nev + 7) // 8
    out = []
    for _ in range(1 + nad):
        b = o; o += 1; ln = varint(); o += ln; out.append(bytes(data[b:o]))
    return out


def check_zero_seam_stream(O, data):
    """The material attribute's seam stream is byte for byte what the oracle's rabs coder (pinned to stock) gives for n_elig zero bits:
    one bit per interior edge."""
    d = O.drc_decode(data)
    n_elig = int((d.opp >= 0).sum()) // 2
    pieces = seam_pieces(data)
    assert len(pieces) == 1 + d.nad and pieces[-1] == O.rabs_encode(np.zeros(n_elig, np.uint8)), (n_elig, pieces[-1][:8].hex())
    if d.nad > 1:                                                               # (the same parse finds the other attributes' streams: same bit count)
        a = d.atts[1]
        assert len(pieces[1]) >= 3


def face_values(d):
    """Per decoded face: the material value of each of its three corners."""
    a = d.atts[len(d.atts) - 1]
    assert a["att_type"] == 4
    return a["vals"][:, 0][a["corner_to_entry"]].reshape(-1, 3)


def check_values(O, data, spans, ids):
    """Check 3: the id of every decoded face is the id of the shell its decoded positions lie in, on all three corners."""
    d = O.drc_decode(data)
    fv = face_values(d)
    assert np.array_equal(fv[:, 0], fv[:, 1]) and np.array_equal(fv[:, 0], fv[:, 2])
    p = d.att("position")
    x = p["float"][p["corner_to_entry"], 0].reshape(-1, 3)
    step = p["range"] / ((1 << p["qbits"]) - 1)
    want = np.full(len(x), -1, np.int64)
    for (lo, hi), mid in zip(spans, ids):
        inside = ((x >= lo - step) & (x <= hi + step)).all(1)
        assert not (inside & (want >= 0)).any()
        want[inside] = mid
    assert (want >= 0).all() and np.array_equal(fv[:, 0], want)
    return d, fv[:, 0]


# ---------------------------------------------------------------------------------------------- the numbered checks
def run_stock_pin(O, cd, extra=()):
    pin = stock_pin(O)
    frames = small_meshes() + list(extra)
    res = cd.encode_mesh_batch([dict(m, face_mat=np.zeros(nfaces(m), np.uint8)) for m in frames])
    base = cd.encode_mesh_batch([plain(m) for m in frames])
    for r, b in zip(res, base):
        d, a = check_stock_row(O, r, pin)
        assert r[a["sec_begin"]:a["sec_end"]] == pin[1]
        check_against_plain(O, r, b)
        check_zero_seam_stream(O, r)


def reference_frame(O):
    """The mesh the oracle decodes out of the recorded 00000.drc, as it is."""
    m = O.drc_decode(open(os.path.join(GOLDEN, "00000.drc"), "rb").read())
    p, u, n = m.att("position"), m.att("tex_coord"), m.att("normal")
    pos = p["float"]
    return dict(pos=pos, idx_pos=p["corner_to_entry"], uv=u["float"], idx_uv=u["corner_to_entry"], nrm=n["float"], idx_nrm=n["corner_to_entry"])


def run_ragged_batch(O, cd):
    """Check 2, second half: NULL entries and a NULL array give the bytes of uvol_encode_mesh_batch, in a ragged batch that mixes frames
    with and without materials, without uv and without normals (att_data_id follows nad)."""
    import uvol
    t, s, g = small_meshes()
    bare = dict(pos=t["pos"], idx_pos=t["idx_pos"])
    no_nrm = dict(pos=g["pos"], idx_pos=g["idx_pos"], uv=g["uv"], idx_uv=g["idx_uv"])
    frames = [dict(t, face_mat=np.full(nfaces(t), 9, np.uint8)), dict(bare, face_mat=np.zeros(nfaces(t), np.uint8)), bare, s, dict(no_nrm, face_mat=np.full(nfaces(g), 255, np.uint8)), no_nrm]
    base = cd.encode_mesh_batch([plain(f) for f in frames])
    res = cd.encode_mesh_batch(frames)
    pin = stock_pin(O)
    for i, (f, r, b) in enumerate(zip(frames, res, base)):
        if f.get("face_mat") is None:
            assert r == b, i
            continue
        nad = 1 + (f.get("uv") is not None) + (f.get("nrm") is not None)
        d, a = check_stock_row(O, r, pin, nad=nad)
        check_against_plain(O, r, b)
        assert np.all(face_values(d) == int(f["face_mat"][0]))
        assert r == cd.encode_mesh(**f), i                                   # ... and a frame's bytes do not depend on its batch
    # a NULL face_material array, and one of NULL entries only: the existing call, through the blocking and the enqueue form
    n = len(frames); meshes = (uvol.Mesh * n)(); keep = []
    for i, f in enumerate(frames):
        m, k = cd._mesh_host(**plain(f)); meshes[i] = m; keep.append(k)
    null_entries = (C.c_void_p * n)()
    for fm in (None, null_entries):
        fn = lambda h, ms, nn, outs, caps, lens, st: cd.L.uvol_encode_mesh_batch_mat(h, ms, fm, nn, 0, outs, caps, lens, st)
        assert cd._run_batch(fn, meshes, n, True) == base
        outs = (C.c_void_p * n)(); caps = (C.c_size_t * n)(); lens = (C.c_size_t * n)(); st = (C.c_int * n)(); bufs = []
        for i in range(n):
            caps[i] = cd.L.uvol_mesh_bound(C.byref(meshes[i])); bufs.append(np.empty(caps[i], np.uint8)); outs[i] = bufs[i].ctypes.data
        assert cd.L.uvol_encode_mesh_batch_mat_async(cd.h, meshes, fm, n, 0, outs, caps, lens, st) == 0 and cd.L.uvol_sync(cd.h) == 0
        assert [bufs[i][:lens[i]].tobytes() for i in range(n)] == base and list(st) == [0] * n


def degenerate_frame():
    """The five-shell frame with a duplicated position and a degenerate face (which the encoder drops) stored FIRST, with an id of its own:
    were the ids not dropped with their faces, every later face would carry its predecessor's."""
    name, m, fm, spans, ids = value_frames()[2]
    m = dict(m)
    npos = len(m["pos"])
    m["pos"] = np.concatenate([m["pos"], m["pos"][:1]])
    for k in ("idx_pos", "idx_uv", "idx_nrm"):
        extra = np.array([0, npos, 5], np.uint32) if k == "idx_pos" else np.array([0, 0, 5], np.uint32)
        m[k] = np.concatenate([extra, m[k]])
    return m, np.concatenate([np.array([99], np.uint8), fm]), spans, ids


def run_values(O, cd):
    """Check 3 (+ check 2's invariants on the same frames); returns the streams for the decoder check."""
    frames = value_frames()
    res = cd.encode_mesh_batch([dict(m, face_mat=fm) for _, m, fm, _, _ in frames])
    base = cd.encode_mesh_batch([plain(m) for _, m, _, _, _ in frames])
    for (name, m, fm, spans, ids), r, b in zip(frames, res, base):
        check_against_plain(O, r, b)
        check_zero_seam_stream(O, r)
        d, got = check_values(O, r, spans, ids)
        assert d.nf == nfaces(m) and sorted(set(got.tolist())) == sorted(set(ids)), name
    m, fm, spans, ids = degenerate_frame()
    r = cd.encode_mesh(**m, face_mat=fm)
    check_against_plain(O, r, cd.encode_mesh(**plain(m)))
    d, got = check_values(O, r, spans, ids)
    assert d.nf == nfaces(m) - 1 and 99 not in got
    return res + [r]


def run_shuffled(O, cd):
    """Check 3, shuffled storage order (run by the tests in a fresh process with the locality relabelling forced on): the ids are permuted
    with the faces, the bytes do not depend on the storage order of ids that follow the faces."""
    name, m, fm, spans, ids = value_frames()[2]
    ms, fms = permute_faces(m, fm, seed=11)
    r = cd.encode_mesh(**ms, face_mat=fms)
    check_against_plain(O, r, cd.encode_mesh(**plain(ms)))
    check_values(O, r, spans, ids)
    md, fmd, spans_d, ids_d = degenerate_frame()
    msd, fmsd = permute_faces(md, fmd, seed=12)
    r = cd.encode_mesh(**msd, face_mat=fmsd)
    d, got = check_values(O, r, spans_d, ids_d)
    assert d.nf == nfaces(md) - 1 and 99 not in got


def run_refusal(O, cd, lib_path=None):
    """Check 4: a torus whose halves carry different ids is refused alone; a _mat call at compression level 0 is refused."""
    import synth, uvol
    t, s, g = small_meshes()
    seam = np.zeros(nfaces(t), np.uint8); seam[nfaces(t) // 2:] = 3
    good0, good2 = dict(s, face_mat=np.full(nfaces(s), 2, np.uint8)), plain(g)
    n = 3; meshes = (uvol.Mesh * n)(); keep = []; fms = []
    for i, f in enumerate([good0, dict(t, face_mat=seam), good2]):
        m, k, fm = cd._mesh_host_mat(**f); meshes[i] = m; keep.append(k); fms.append(fm)
    mats = cd._mat_ptrs(fms)
    outs = (C.c_void_p * n)(); caps = (C.c_size_t * n)(); lens = (C.c_size_t * n)(); st = (C.c_int * n)(); bufs = []
    for i in range(n):
        caps[i] = cd.L.uvol_mesh_bound_mat(C.byref(meshes[i])); bufs.append(np.empty(caps[i], np.uint8)); outs[i] = bufs[i].ctypes.data
    assert cd.L.uvol_encode_mesh_batch_mat(cd.h, meshes, mats, n, 0, outs, caps, lens, st) == 0
    assert list(st) == [uvol.UVOL_OK, uvol.UVOL_E_UNSUPPORTED, uvol.UVOL_OK]
    assert "mesh 1" in cd.error() and "material" in cd.error()
    assert bufs[0][:lens[0]].tobytes() == cd.encode_mesh(**good0) and bufs[2][:lens[2]].tobytes() == cd.encode_mesh(**good2)
    res = cd.encode_mesh_batch([good0, dict(t, face_mat=seam), good2], raise_on_error=False)
    assert res[1] is None and res[0] == cd.encode_mesh(**good0) and res[2] == cd.encode_mesh(**good2)
    c0 = uvol.Codec(lib_path=lib_path, DRACO_COMPRESSION_LEVEL=0) if lib_path else uvol.Codec(device=0, DRACO_COMPRESSION_LEVEL=0)
    try:
        try:
            c0.encode_mesh_batch([good0])
            raise AssertionError("a _mat call at compression level 0 must be refused")
        except uvol.UvolError as e:
            assert "rc=%d" % uvol.UVOL_E_UNSUPPORTED in str(e)
        assert c0.encode_mesh(**plain(s))[:5] == b"DRACO"                    # ... the same call without ids is the existing one
    finally:
        c0.close()


def decode_raw(cd, mem, files, on_device, with_mat):
    """uvol_decode_mesh_batch[_dev] / uvol_decode_mesh_batch_mat through ctypes -> list of dicts of host arrays (+ face_mat, has_mat)."""
    import uvol
    n = len(files); files = [bytes(f) for f in files]
    metas = (uvol.DecodedMesh * n)(); hb = []; fmp = (C.c_void_p * n)(); hm = (C.c_int * n)(*([7] * n)); fbuf = []
    spec = (("pos", np.float32, 3), ("uv", np.float32, 2), ("nrm", np.float32, 3), ("idx_pos", np.uint32, 3), ("idx_uv", np.uint32, 3), ("idx_nrm", np.uint32, 3))
    for i, f in enumerate(files):
        nf, mv = cd.drc_info(f); metas[i].cap_faces = nf; metas[i].cap_values = mv; row = {}
        for k, dt, w in spec:
            cnt = w * (nf if k.startswith("idx") else mv)
            if on_device: row[k] = mem.alloc(4 * cnt)
            else: a = np.zeros(cnt, dt); row[k] = a
            setattr(metas[i], k, row[k] if on_device else row[k].ctypes.data)
        hb.append(row)
        if on_device: fbuf.append(mem.to_dev(np.full(nf, 0xEE, np.uint8))); fmp[i] = fbuf[i]
        else: fbuf.append(np.full(nf, 0xEE, np.uint8)); fmp[i] = fbuf[i].ctypes.data
    fp = (C.c_char_p * n)(*files); ln = (C.c_size_t * n)(*[len(f) for f in files]); st = (C.c_int * n)()
    if with_mat:
        rc = cd.L.uvol_decode_mesh_batch_mat(cd.h, fp, ln, n, 1 if on_device else 0, metas, fmp, hm, st)
    else:
        rc = (cd.L.uvol_decode_mesh_batch_dev if on_device else cd.L.uvol_decode_mesh_batch)(cd.h, fp, ln, n, metas, st)
    assert rc == 0 and list(st) == [0] * n, (rc, list(st), cd.error())
    out = []
    for i in range(n):
        m = metas[i]; cnt = dict(pos=3 * m.n_pos, uv=2 * m.n_uv, nrm=3 * m.n_nrm, idx_pos=3 * m.n_faces, idx_uv=3 * m.n_faces if m.n_uv else 0, idx_nrm=3 * m.n_faces if m.n_nrm else 0)
        r = {k: (mem.to_host(hb[i][k], dt, cnt[k]) if on_device else hb[i][k][:cnt[k]].copy()) for k, dt, w in spec}
        r["n_faces"] = m.n_faces
        if with_mat:
            r["has_mat"] = hm[i]
            r["face_mat"] = mem.to_host(fbuf[i], np.uint8, m.n_faces) if on_device else fbuf[i][:m.n_faces].copy()
        out.append(r)
    return out


def run_decoder(O, cd, mem, streams):
    """Check 5: the two recorded files, the streams of check 3 and a three-decoder stream, host and device output form."""
    golden = [open(os.path.join(GOLDEN, nme), "rb").read() for nme in ("00000.drc", "00075.drc")]
    three = cd.encode_mesh(**plain(small_meshes()[0]))
    files = golden + list(streams) + [three]
    for on_device in (False, True):
        got = decode_raw(cd, mem, files, on_device, True)
        ref = decode_raw(cd, mem, files, on_device, False)
        for i, (g, r, f) in enumerate(zip(got, ref, files)):
            for k in ("pos", "uv", "nrm", "idx_pos", "idx_uv", "idx_nrm"):
                assert np.array_equal(g[k].view(np.uint32), r[k].view(np.uint32)), (i, k)
            if i == len(files) - 1:
                assert g["has_mat"] == 0 and np.all(g["face_mat"] == 0xEE)      # no material: flag 0, the buffer is left alone
                continue
            assert g["has_mat"] == 1, i
            want = face_values(O.drc_decode(f))[:, 0]
            assert g["n_faces"] == len(want) and np.array_equal(g["face_mat"], want), i
            if i < 2:
                assert np.all(g["face_mat"] == 0)
        mem.free_all()
    assert "face_mat" not in cd.decode_mesh_batch(files[:1])[0]                 # the binding: opt-in, then face_mat or None
    py = cd.decode_mesh_batch(files, materials=True)
    assert py[-1]["face_mat"] is None and np.all(py[0]["face_mat"] == 0) and np.array_equal(py[2]["face_mat"], face_values(O.drc_decode(files[2]))[:, 0])


OBJ_MATERIALS = "\r\n".join([
    "mtllib scene.mtl", "v 0 0 0", "v 1 0 0", "v 1 1 0", "v 0 1 0", "v 2 0 0", "v 2 1 0", "v 3 0.5 0", "v 0 2 0", "v 1 2 0",
    "f 1 2 3", "f 1 3 4",                                   # ahead of the first usemtl: id 0 ...
    "usemtl skin   ", "f 2 5 6 3",                          # ... which is also the first NAME's id (first appearance); a quad, trailing blanks
    "  usemtl\tcloth", "f 5 7 6", "f 4 3 9 8 1",            # blanks ahead of the keyword, a tab behind it; a pentagon
    "usemtl metal", "usemtl skin", "f 3 6 9",               # a name that sets nothing, a name used twice
    "usemtl metal \t ", "f 6 7 9", ""])
OBJ_MATERIAL_IDS = [0, 0, 0, 0, 1, 1, 1, 1, 0, 2]


def host_materials(path):
    """read_obj's material ids (libuvolhost.so test hook): array, or None when the file has no usemtl line."""
    import subprocess
    pkg = os.path.join(ROOT, "universal-volumetric_amd")
    subprocess.check_call(["make", "-s", "-C", pkg, "libuvolhost.so"])
    H = C.CDLL(os.path.join(pkg, "libuvolhost.so"))
    H.uvolh_read_obj_materials.restype = C.c_long; H.uvolh_read_obj_materials.argtypes = [C.c_char_p, C.c_void_p, C.c_size_t]
    buf = np.zeros(1 << 20, np.uint8)
    n = H.uvolh_read_obj_materials(str(path).encode(), buf.ctypes.data, buf.size)
    assert n >= 0
    return buf[:n].copy() if n else None


def run_ingest(O, cd, mem, tmp_path):
    """Check 6: read_obj and the device parser give the same, expected ids; a file without usemtl yields NULL and the arrays of
    uvol_parse_obj_batch_dev; the parsed frames go straight into the encoder."""
    import uvol
    from test_hipemu_geom import _obj_texts
    p = tmp_path / "mat.obj"; p.write_bytes(OBJ_MATERIALS.encode())
    # many names in a text of several 4 KiB tiles: usemtl lines ranked across workgroups
    rng = np.random.default_rng(5); big = ["v %d %d 0" % (i % 97, i // 97) for i in range(400)]; want_big = []; names = {}
    for k in range(900):
        if k % 7 == 3:
            nm = "m%d" % int(rng.integers(0, 40)); big.append("usemtl " + nm + " " * int(rng.integers(0, 3))); cur = names.setdefault(nm, len(names))
        nc = int(rng.integers(3, 7)); big.append("f " + " ".join(str(int(x) + 1) for x in rng.integers(0, 400, nc)))
        want_big += [names[nm] if k >= 3 else 0] * (nc - 2)
    pb = tmp_path / "big.obj"; pb.write_text("\n".join(big) + "\n")
    plain_paths = _obj_texts(tmp_path)[:2]                                      # (a.obj has a mtllib line and no usemtl)
    paths = [p, pb] + plain_paths
    texts = [open(q, "rb").read() for q in paths]; n = len(texts)
    tp = (C.c_char_p * n)(*texts); ln = (C.c_size_t * n)(*[len(t) for t in texts]); meshes = (uvol.Mesh * n)(); st = (C.c_int * n)(); fm = (C.c_void_p * n)(*([1] * n))
    assert cd.L.uvol_parse_obj_batch_dev_mat(cd.h, tp, ln, n, 0, meshes, fm, st) == 0 and list(st) == [0] * n, cd.error()
    for i, (q, want) in enumerate(zip(paths, [OBJ_MATERIAL_IDS, want_big, None, None])):
        h = host_materials(q)
        if want is None:
            assert h is None and not fm[i], q
            continue
        assert meshes[i].n_faces == len(want) and fm[i]
        d = mem.to_host(fm[i], np.uint8, meshes[i].n_faces)
        assert np.array_equal(h, np.array(want, np.uint8)) and np.array_equal(d, h), (q, h.tolist()[:20], d.tolist()[:20])
    # the same mesh arrays as the entry point without materials (parsed into the other slot)
    ref, st2 = cd.parse_obj_batch_dev(texts, slot=1)
    assert st2 == [0] * n
    for a, b in zip(meshes, ref):
        assert (a.n_pos, a.n_uv, a.n_nrm, a.n_faces, bool(a.uv), bool(a.nrm)) == (b.n_pos, b.n_uv, b.n_nrm, b.n_faces, bool(b.uv), bool(b.nrm))
        assert np.array_equal(mem.to_host(a.pos, np.uint32, 3 * a.n_pos), mem.to_host(b.pos, np.uint32, 3 * b.n_pos)) and np.array_equal(mem.to_host(a.idx_pos, np.uint32, 3 * a.n_faces), mem.to_host(b.idx_pos, np.uint32, 3 * b.n_faces))
    # ids that follow connected components, parsed on the device and encoded from HBM: the values come back
    name, m, fmat, spans, ids = value_frames()[2]
    lines = ["v %.9g %.9g %.9g" % tuple(float(x) for x in v) for v in m["pos"]] + ["vt %.9g %.9g" % tuple(float(x) for x in v) for v in m["uv"]] + ["vn %.9g %.9g %.9g" % tuple(float(x) for x in v) for v in m["nrm"]]
    ip, iu, inn = (m[k].reshape(-1, 3) + 1 for k in ("idx_pos", "idx_uv", "idx_nrm")); last = None; order = []
    for f in range(nfaces(m)):
        if fmat[f] != last:
            lines.append("usemtl id%d" % fmat[f]); last = fmat[f]
            if int(last) not in order: order.append(int(last))
        lines.append("f " + " ".join("%d/%d/%d" % (ip[f][k], iu[f][k], inn[f][k]) for k in range(3)))
    text = ("\n".join(lines) + "\n").encode()
    tp = (C.c_char_p * 1)(text); ln = (C.c_size_t * 1)(len(text)); ms = (uvol.Mesh * 1)(); st = (C.c_int * 1)(); fm1 = (C.c_void_p * 1)()
    assert cd.L.uvol_parse_obj_batch_dev_mat(cd.h, tp, ln, 1, 0, ms, fm1, st) == 0 and st[0] == 0 and fm1[0]
    r = cd.encode_mesh_batch_dev_mat(ms, [fm1[0]])[0]
    check_values(O, r, spans, [order.index(i) for i in ids])                    # (ids by first appearance of the name)
    pin = stock_pin(O); check_stock_row(O, r, pin)
