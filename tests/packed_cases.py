"""Checks of the packed render-ready mesh decode (uvol_decode_mesh_batch_packed: one index per corner, one 16-byte record of the file's own
integers per point, with material ids) shared by tests/test_hipemu_packed.py (host emulation of the kernels) and tests/test_gpu_packed.py
(MI355X).  Every check takes the oracle module, a uvol.Codec and, where device memory is involved, a Mem of tests/material_cases.py.

The expected result is built here, in NumPy, from the ORACLE decoder's output alone, the way tests/points_cases.py::reference builds the
float form's: the tuples (corner_to_entry of position, tex-coord, normal) are stacked, np.unique(axis=0) finds the distinct ones and the
unique rows are re-ranked by the corner of their first appearance.  The record fields are then taken from the oracle's `vals` (positions,
tex-coords, material), its `float` normals (times 127, rounded to nearest even) and its `minv` / `range` / `qbits`.  Records are compared
as raw bytes, the transform bit for bit.  The record layout is declared HERE, from the interface's table, not taken from the binding."""
import ctypes as C
import os
import numpy as np
from conftest import GOLDEN
import material_cases as MC
import points_cases as PC

U32 = np.uint32
F32 = np.float32
# bytes 0-5 uint16 px py pz | 6-7 uint16 material | 8-11 uint16 u v | 12-15 int8 nx ny nz 0, little endian
RECORD = np.dtype([("pos", "<u2", 3), ("material", "<u2"), ("uv", "<u2", 2), ("nrm", "i1", 4)])
assert RECORD.itemsize == 16
META = ("n_faces", "n_points", "has_uv", "has_nrm", "has_material", "pos_bits", "uv_bits")


def golden(*names):
    return [open(os.path.join(GOLDEN, n), "rb").read() for n in names]


def material_attribute(d):
    """The oracle's row of the attribute uvol_decode_mesh_batch_mat reads, or None: GENERIC (4) UINT8 (2), one component, a vertex
    attribute (decoder type 0, hence on the base corner table) with plain integer values (seq_type 1) of an edgebreaker file."""
    if d.method != 1:
        return None
    for a in d.atts:
        if a["att_type"] == 4 and a["data_type"] == 2 and a["ncomp"] == 1 and a["dec_type"] == 0 and a["seq_type"] == 1:
            return a
    return None


def scale_of(a):
    return F32(a["range"]) / F32(2 ** a["qbits"] - 1)


def reference(O, data):
    """Expected result of one file, from the oracle decoder alone."""
    d = O.drc_decode(data)
    atts = {key: d.att(name) for name, key, _ in PC.NAMES}
    assert atts["pos"] is not None
    present = [k for k in ("pos", "uv", "nrm") if atts[k] is not None]
    keys = np.stack([atts[k]["corner_to_entry"].astype(np.int64) for k in present], axis=1)
    uniq, first, inv = np.unique(keys, axis=0, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")                 # unique rows in the order of their first corner
    rank = np.empty(len(order), np.int64); rank[order] = np.arange(len(order))
    rows = dict(zip(present, uniq[order].T)); first_corner = first[order]
    n = len(order)
    rec = np.zeros(n, RECORD)
    rec["pos"] = atts["pos"]["vals"][rows["pos"], :3]
    if atts["uv"] is not None: rec["uv"] = atts["uv"]["vals"][rows["uv"], :2]
    if atts["nrm"] is not None: rec["nrm"][:, :3] = np.rint(atts["nrm"]["float"][rows["nrm"]] * F32(127)).astype(np.int8)
    mat = material_attribute(d)
    if mat is not None: rec["material"] = mat["vals"][:, 0][mat["corner_to_entry"][first_corner]]
    ref = dict(n_faces=d.nf, n_points=n, index=rank[np.asarray(inv).reshape(-1)].astype(U32), records=rec, has_uv=atts["uv"] is not None, has_nrm=atts["nrm"] is not None,
               has_material=mat is not None, pos_bits=atts["pos"]["qbits"], uv_bits=atts["uv"]["qbits"] if atts["uv"] is not None else 0,
               pos_min=np.array(atts["pos"]["minv"][:3], F32), pos_scale=scale_of(atts["pos"]),
               uv_min=np.array(atts["uv"]["minv"][:2], F32) if atts["uv"] is not None else np.zeros(2, F32), uv_scale=scale_of(atts["uv"]) if atts["uv"] is not None else F32(0))
    return ref


def raw(records):
    return np.ascontiguousarray(records).view(np.uint8).reshape(-1, 16)


def check_frame(ref, got, tag=""):
    assert got is not None, tag
    assert tuple(int(got[k]) for k in META) == tuple(int(ref[k]) for k in META), (tag, [got[k] for k in META], [ref[k] for k in META])
    for k in ("pos_min", "pos_scale", "uv_min", "uv_scale"):
        assert PC.same_bits(np.atleast_1d(np.asarray(got[k], F32)), np.atleast_1d(np.asarray(ref[k], F32))), (tag, k, got[k], ref[k])
    assert np.array_equal(np.asarray(got["index"]), ref["index"]), tag
    a, b = raw(got["records"]), raw(ref["records"])
    assert a.shape == b.shape, (tag, a.shape, b.shape)
    bad = np.flatnonzero((a != b).any(1))
    assert len(bad) == 0, (tag, len(bad), bad[:4], a[bad[:2]], b[bad[:2]])


def check_dequant_formula(O, data):
    """CPU only: NumPy's minv + q * scale in float32 - the product rounded, then the sum: NumPy never fuses the two - is the oracle's
    `float` bit for bit, for positions and tex-coords.  (The oracle is built with -ffp-contract=off, oracle/Makefile: no fused form.)
    This is the formula include/uvol_codec.h documents for the packed records."""
    d = O.drc_decode(data)
    for name in ("position", "tex_coord"):
        a = d.att(name)
        if a is None: continue
        assert a["seq_type"] == 2
        q = a["vals"].astype(F32); s = scale_of(a); mn = np.array(a["minv"][:a["ncomp"]], F32)
        prod = q * s; val = mn[None, :] + prod
        assert val.dtype == F32 and PC.same_bits(val, a["float"]), name


# ---------------------------------------------------------------------------------------------- device outputs
def decode_dev(cd, mem, files, caps=None, fill=None):
    """Device outputs through `mem` -> (statuses, metas, host copies as decode_mesh_batch_packed returns them, device pointers)."""
    import uvol
    n = len(files); metas = (uvol.PackedPoints * n)(); ptr = []
    for i, f in enumerate(files):
        nf, mv = cd.drc_info(f) if caps is None else caps[i]
        metas[i].cap_faces = nf; metas[i].cap_points = mv
        row = dict(index=mem.to_dev(np.full(12 * nf, fill, np.uint8)) if fill is not None else mem.alloc(12 * nf),
                   records=mem.to_dev(np.full(16 * mv, fill, np.uint8)) if fill is not None else mem.alloc(16 * mv), nf=nf, mv=mv)
        assert row["records"] % 16 == 0
        metas[i].records = row["records"]; metas[i].index = row["index"]; ptr.append(row)
    st = cd.decode_mesh_batch_packed(files, on_device=True, metas=metas)
    out = []
    for i in range(n):
        m = metas[i]
        if st[i] != 0:
            out.append(None); continue
        out.append(dict(uvol.packed_meta(m), index=mem.to_host(ptr[i]["index"], U32, 3 * m.n_faces), records=mem.to_host(ptr[i]["records"], np.uint8, 16 * m.n_points).reshape(-1, 16)))
    return st, metas, out, ptr


# ---------------------------------------------------------------------------------------------- checks 1 and 2
def run_recorded(O, cd, files, batch=None):
    """Check 1: recorded files, in batches of `batch`: records, index, counts, flags and transform are the reference's.  Check 2 on the
    same files: index and n_points are those of uvol_decode_mesh_batch_points.  Every recorded file carries the (all-zero) material
    attribute and 11 / 10 quantisation bits."""
    batch = batch or len(files)
    for b0 in range(0, len(files), batch):
        part = files[b0:b0 + batch]
        got = cd.decode_mesh_batch_packed(part)
        pts = cd.decode_mesh_batch_points(part, layout="interleaved")
        assert len(got) == len(part)
        for i, (f, g, p) in enumerate(zip(part, got, pts)):
            r = reference(O, f)
            check_frame(r, g, b0 + i)
            assert g["has_material"] and g["has_uv"] and g["has_nrm"] and (g["pos_bits"], g["uv_bits"]) == (11, 10), b0 + i
            assert g["n_points"] == p["n_points"] and np.array_equal(g["index"], p["index"]), b0 + i
    return len(files)


# ---------------------------------------------------------------------------------------------- check 3
def run_subsets(O, cd, cd0):
    """Check 3: the streams of points_cases.subset_streams (positions only, + uv, + normals, all three with seams, a polygon soup, two
    `-cl 0` streams): absent slots zero, has_uv / has_nrm / uv_bits right, no material; the same points as the float form (check 2)."""
    streams = PC.subset_streams(cd, cd0)
    files = [f for _, f in streams]
    want_has = dict(pos_only=(False, False), pos_uv=(True, False), pos_nrm=(False, True), all_three_seams=(True, True), all_three_grid_holes=(True, True),
                    soup=(True, True), cl0_all_three=(True, True), cl0_pos_uv=(True, False))
    assert O.drc_decode(files[-2]).method == 0 and O.drc_decode(files[3]).method == 1          # the sequential stream is one
    refs = [reference(O, f) for f in files]
    assert any(r["n_points"] % 256 for r in refs) and any(r["n_points"] > 256 for r in refs)    # more than one block, and a ragged last block
    got = cd.decode_mesh_batch_packed(files)
    pts = cd.decode_mesh_batch_points(files)
    for (name, _), r, g, p in zip(streams, refs, got, pts):
        assert (g["has_uv"], g["has_nrm"]) == want_has[name] and not g["has_material"], name
        assert g["uv_bits"] == (10 if g["has_uv"] else 0) and g["pos_bits"] == 11, name
        check_frame(r, g, name)
        rec = np.asarray(g["records"]).view(RECORD).reshape(-1)
        assert not rec["material"].any() and not rec["nrm"][:, 3].any(), name
        if not g["has_uv"]: assert not rec["uv"].any() and g["uv_scale"] == 0 and not np.any(g["uv_min"]), name
        if not g["has_nrm"]: assert not rec["nrm"].any(), name
        assert g["n_points"] == p["n_points"] and np.array_equal(g["index"], p["index"]), name
    return files


# ---------------------------------------------------------------------------------------------- check 4
def material_frames():
    """(name, mesh, face_mat): multi-shell meshes, three or more ids that follow the connected components."""
    import synth
    t, g, s2 = synth.torus_mesh(), synth.grid_mesh(), synth.sphere_mesh(24, 13, charts=(3, 2), crease=False)
    name, m5, fm5, _, _ = MC.value_frames()[2]                                  # five shells, ids 0 7 200 31 7
    m3, fm3, _ = MC.shells([t, g, s2], [3, 255, 1])
    return [(name, m5, fm5), ("three_shells", m3, fm3)]


def run_materials(O, cd):
    """Check 4: every point's material is the oracle's value, has_material is 1; the same mesh without ids gives has_material 0 and a zero
    slot, everything else equal; the material at each face's first corner equals uvol_decode_mesh_batch_mat's per-face ids."""
    frames = material_frames()
    with_ids = cd.encode_mesh_batch([dict(m, face_mat=fm) for _, m, fm in frames])
    without = cd.encode_mesh_batch([MC.plain(m) for _, m, _ in frames])
    got = cd.decode_mesh_batch_packed(with_ids + without)
    facemat = cd.decode_mesh_batch(with_ids, materials=True)
    k = len(frames)
    for i, (name, m, fm) in enumerate(frames):
        r = reference(O, with_ids[i]); g = got[i]
        assert r["has_material"] and len(set(r["records"]["material"].tolist())) >= 3, name
        check_frame(r, g, name)
        rec = np.asarray(g["records"]).view(RECORD).reshape(-1)
        assert g["has_material"] and set(rec["material"].tolist()) == set(int(x) for x in fm), name
        per_face = rec["material"][np.asarray(g["index"])[0::3]]
        assert np.array_equal(per_face, facemat[i]["face_mat"]), name
        corners = rec["material"][np.asarray(g["index"])].reshape(-1, 3)           # no point is shared by two materials
        assert np.array_equal(corners[:, 0], corners[:, 1]) and np.array_equal(corners[:, 0], corners[:, 2]), name
        r0 = reference(O, without[i]); g0 = got[k + i]
        assert not r0["has_material"]
        check_frame(r0, g0, name + " without ids")
        rec0 = np.asarray(g0["records"]).view(RECORD).reshape(-1)
        assert not g0["has_material"] and not rec0["material"].any(), name
        plain = rec.copy(); plain["material"] = 0
        assert np.array_equal(raw(plain), raw(rec0)) and np.array_equal(g["index"], g0["index"]), name
    return with_ids


# ---------------------------------------------------------------------------------------------- check 5
def run_ragged(O, cd, cd0, mem):
    """Check 5: a truncated file, a foreign file, a frame one point short, a frame one face short and the long-fan mesh fail alone with
    their codes, the needed counts are reported, the neighbours are byte-correct.  A misaligned DEVICE records pointer fails the whole
    call with UVOL_E_INVALID and nothing is written."""
    import uvol
    good = [f for _, f in PC.subset_streams(cd, cd0)] + [run_materials_stream(cd)]
    trunc = good[3][:len(good[3]) * 2 // 3]; foreign = b"OBJ? no: not a Draco file at all " * 8
    long_fan = cd0.encode_mesh(**PC.disk_mesh(4200))
    files = [good[0], trunc, good[3], foreign, good[8], good[4], good[6], good[1], long_fan, good[5], good[7]]
    TRUNC, FOREIGN, SHORT, FEW_FACES, FAN = 1, 3, 5, 7, 8
    failing = (TRUNC, FOREIGN, SHORT, FEW_FACES, FAN)
    refs = {i: reference(O, f) for i, f in enumerate(files) if i not in (TRUNC, FOREIGN, FAN)}
    metas = (uvol.PackedPoints * len(files))()
    for i, f in enumerate(files):
        if i == FOREIGN:
            metas[i].cap_faces = 100; metas[i].cap_points = 300; continue
        nf, mv = cd.drc_info(f); metas[i].cap_faces = nf; metas[i].cap_points = mv
    metas[SHORT].cap_points = refs[SHORT]["n_points"] - 1
    metas[FEW_FACES].cap_faces = refs[FEW_FACES]["n_faces"] - 1
    st = []
    got = cd.decode_mesh_batch_packed(files, raise_on_error=False, metas=metas, status_out=st)
    want = {TRUNC: uvol.UVOL_E_ENCODE, FOREIGN: uvol.UVOL_E_INVALID, SHORT: uvol.UVOL_E_NOSPACE, FEW_FACES: uvol.UVOL_E_NOSPACE, FAN: uvol.UVOL_E_UNSUPPORTED}
    assert st == [want.get(i, 0) for i in range(len(files))], st
    assert metas[SHORT].n_points == refs[SHORT]["n_points"] and metas[FEW_FACES].n_faces == refs[FEW_FACES]["n_faces"]
    for i in range(len(files)):
        if i in failing:
            assert got[i] is None; continue
        check_frame(refs[i], got[i], i)
    # the capacity that is exactly enough is enough
    two = (uvol.PackedPoints * 2)()
    two[0].cap_faces = metas[SHORT].cap_faces; two[0].cap_points = refs[SHORT]["n_points"]; two[1].cap_faces = refs[FEW_FACES]["n_faces"]; two[1].cap_points = metas[FEW_FACES].cap_points
    got = cd.decode_mesh_batch_packed([files[SHORT], files[FEW_FACES]], metas=two)
    check_frame(refs[SHORT], got[0]); check_frame(refs[FEW_FACES], got[1])
    # device outputs: the short frame and the long fan leave their buffers alone, the neighbours are written
    sub = [files[0], files[SHORT], files[FAN], files[2]]
    caps = [cd.drc_info(f) for f in sub]; caps[1] = (caps[1][0], refs[SHORT]["n_points"] - 1)
    st, dm, dev, ptr = decode_dev(cd, mem, sub, caps, fill=0xEE)
    assert st == [0, uvol.UVOL_E_NOSPACE, uvol.UVOL_E_UNSUPPORTED, 0] and dm[1].n_points == refs[SHORT]["n_points"]
    check_frame(refs[0], dev[0], "dev 0"); check_frame(refs[2], dev[3], "dev 3")
    for i in (1, 2):
        assert np.all(mem.to_host(ptr[i]["records"], np.uint8, 16 * ptr[i]["mv"]) == 0xEE) and np.all(mem.to_host(ptr[i]["index"], np.uint8, 12 * ptr[i]["nf"]) == 0xEE), i
    # a misaligned device records pointer in ANY frame: the whole call is refused, nothing runs
    n = 2; fl = [files[0], files[2]]; m2 = (uvol.PackedPoints * n)(); rows = []
    for i, f in enumerate(fl):
        nf, mv = cd.drc_info(f); m2[i].cap_faces = nf; m2[i].cap_points = mv
        rows.append((mem.to_dev(np.full(16 * mv + 16, 0xEE, np.uint8)), mem.to_dev(np.full(12 * nf, 0xEE, np.uint8)), nf, mv))
        m2[i].records = rows[i][0] + (8 if i == 1 else 0); m2[i].index = rows[i][1]
    fp = (C.c_char_p * n)(*fl); ln = (C.c_size_t * n)(*[len(f) for f in fl]); stc = (C.c_int * n)()
    assert cd.L.uvol_decode_mesh_batch_packed(cd.h, fp, ln, n, 1, m2, stc) == uvol.UVOL_E_INVALID and "aligned" in cd.error()
    for rp, ip, nf, mv in rows:
        assert np.all(mem.to_host(rp, np.uint8, 16 * mv + 16) == 0xEE) and np.all(mem.to_host(ip, np.uint8, 12 * nf) == 0xEE)
    # without a status array the call reports the worst frame; a lone good frame is UVOL_OK
    m2[1].records = rows[1][0]
    fl2 = [files[0], foreign]; fp = (C.c_char_p * n)(*fl2); ln = (C.c_size_t * n)(*[len(f) for f in fl2])
    assert cd.L.uvol_decode_mesh_batch_packed(cd.h, fp, ln, n, 1, m2, None) == uvol.UVOL_E_INVALID
    assert cd.L.uvol_decode_mesh_batch_packed(cd.h, fp, ln, 1, 1, m2, None) == uvol.UVOL_OK and m2[0].n_points == refs[0]["n_points"]
    mem.free_all()


def run_materials_stream(cd):
    """One stream that carries material ids (a neighbour for the ragged batch)."""
    name, m, fm = material_frames()[1]
    return cd.encode_mesh(**m, face_mat=fm)


# ---------------------------------------------------------------------------------------------- check 6
def wide_stream(O):
    """A stream that declares 17 quantisation bits for its positions.  The oracle encoder refuses qp = 17 (oracle/drc_enc.c takes 1 .. 16;
    asserted below), so the case is built from the widest setting it does accept: a qp = 16 stream - whose integers reach 65535, the whole
    uint16 range - and a copy of it whose quantisation-bits byte, the one behind the position attribute's `range`, is rewritten to 17.
    The attribute's integers do not depend on that byte (it only enters the dequantisation step), and the oracle decoder reads the copy
    back with qbits 17 and the same integers.  -> (the 16-bit stream, the 17-bit copy)"""
    import struct
    t = MC.small_meshes()[0]
    args = (t["pos"], t["idx_pos"], t["uv"], t["idx_uv"], t["nrm"], t["idx_nrm"])
    try:
        O.drc_encode(*args, qp=17)
        raise AssertionError("the oracle encoder now accepts qp=17: encode the case with it")
    except ValueError:
        pass
    data = O.drc_encode(*args, qp=16)
    d = O.drc_decode(data); a = d.att("position")
    assert d.leftover == 0 and a["qbits"] == 16 and a["seq_type"] == 2 and int(a["vals"].max()) == 65535 and d.nf == MC.nfaces(t)
    tail = struct.pack("<f", a["range"]) + bytes([16])
    assert data.count(tail) == 1
    o = data.index(tail) + 4
    wide = data[:o] + bytes([17]) + data[o + 1:]
    w = O.drc_decode(wide); b = w.att("position")
    assert w.leftover == 0 and b["qbits"] == 17 and np.array_equal(b["vals"], a["vals"]) and b["range"] == a["range"]
    return data, wide


def run_wide_quantisation(O, cd):
    """Check 6: positions declared as 17-bit: UVOL_E_UNSUPPORTED for that frame alone, uvol_last_error names the position attribute; the
    other entry points still decode the file, the neighbours come out byte-correct.  The 16-bit stream beside it is the widest the
    records hold: it decodes, integers up to 65535 unchanged."""
    import uvol
    full16, wide = wide_stream(O); good = cd.encode_mesh(**MC.plain(MC.small_meshes()[1]))
    files = [good, wide, full16, good]
    PC.check_old_decode(O, wide, cd.decode_mesh_batch([wide])[0])
    PC.check_frame(PC.reference(O, wide), cd.decode_mesh_batch_points([wide])[0], "planar")
    st = []
    got = cd.decode_mesh_batch_packed(files, raise_on_error=False, status_out=st)
    assert st == [0, uvol.UVOL_E_UNSUPPORTED, 0, 0], st
    assert "position" in cd.error() and "17" in cd.error(), cd.error()
    assert got[1] is None
    r = reference(O, good)
    check_frame(r, got[0]); check_frame(r, got[3])
    r16 = reference(O, full16)
    assert r16["pos_bits"] == 16 and int(r16["records"]["pos"].max()) == 65535
    check_frame(r16, got[2])


# ---------------------------------------------------------------------------------------------- check 7
def run_memory_forms(O, cd, cd0, mem, lib_path=None, extra=()):
    """Check 7: device outputs, pageable host outputs and outputs in a PinnedArena: all the reference's."""
    import uvol
    files = [f for _, f in PC.subset_streams(cd, cd0)] + [run_materials_stream(cd)] + list(extra)
    refs = [reference(O, f) for f in files]
    st, _, dev, _ = decode_dev(cd, mem, files)
    assert st == [0] * len(files)
    host = cd.decode_mesh_batch_packed(files)
    ar = uvol.PinnedArena(cd.points_arena_bytes(files), lib_path=lib_path)
    try:
        pinned = cd.decode_mesh_batch_packed(files, arena=ar)
        for i, r in enumerate(refs):
            for form, got in (("device", dev), ("host", host), ("pinned", pinned)):
                check_frame(r, got[i], (form, i))
    finally:
        del pinned; ar.close()
    mem.free_all()


# ---------------------------------------------------------------------------------------------- check 8
PACKED_GROUPS = {"geodec.k8_keys_packed", "geodec.k9_weld_packed"}


def run_existing_untouched(O, cd, files):
    """Check 8: after packed calls on the context, uvol_decode_mesh_batch, _mat and _points still equal their references and record none
    of the packed path's kernel groups; a packed call records its own two groups and neither the float write-out group
    (geodec.k8_finish) nor the float weld's."""
    groups = lambda: {g["name"] for g in cd.profile_report() if g["launches"] > 0}
    cd.decode_mesh_batch_packed(files)
    cd.profile(True); cd.profile_reset()
    try:
        cd.decode_mesh_batch_packed(files)
        mine = groups()
        assert PACKED_GROUPS <= mine and "geodec.k8_finish" not in mine and "geodec.k9_weld" not in mine, mine
        cd.profile_reset()
        for f, g in zip(files, cd.decode_mesh_batch(files)):
            PC.check_old_decode(O, f, g)
        mats = MC.decode_raw(cd, MC.HostMem(), files, False, True)                                  # the _mat form (host outputs)
        for f, g in zip(files, mats):
            d = O.drc_decode(f); a = material_attribute(d)
            assert g["has_mat"] == (a is not None)
            if a is not None: assert np.array_equal(g["face_mat"], MC.face_values(d)[:, 0])
        for layout in ("planar", "interleaved"):
            for f, g in zip(files, cd.decode_mesh_batch_points(files, layout=layout)):
                PC.check_frame(PC.reference(O, f), g, layout)
        theirs = groups()
        assert {"geodec.k8_finish", "geodec.k9_weld"} <= theirs and not (theirs & PACKED_GROUPS), theirs
        assert mine - PACKED_GROUPS == theirs - {"geodec.k8_finish", "geodec.k9_weld"}, (mine, theirs)   # every other stage is shared
    finally:
        cd.profile(False)
