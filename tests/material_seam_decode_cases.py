"""Checks of the DECODE side of the corner-form material attribute (files written with `uvol_params.material_seams = 1`, read back by
uvol_decode_mesh_batch_mat, _packed and the plain entry points), shared by tests/test_hipemu_material_seam_decode.py (host emulation of the
kernels) and tests/test_gpu_material_seam_decode.py (MI355X).  Every check takes the oracle module, a uvol.Codec created with
material_seams=1 (it writes the files and reads them back) and, where device memory is involved, a Mem of tests/material_cases.py.

The judge of every file is the repository's oracle DECODER (oracle.drc_decode), which reads attribute-data slots generically:
material_cases.face_values gives the per-corner values, points_cases.check_old_decode compares positions, tex-coords and normals.  The
packed reference is built here in NumPy from the oracle's output alone: the tuples (position entry, tex-coord entry, normal entry, corner
material) are numbered by first appearance in corner order.

The material sits on the seam-cut table of its OWN attribute-data slot: slot 2 for a frame with tex-coords and normals (a third table, the
pass of csrc/geo_mattab_dec.hpp), slot 1 without tex-coords, slot 0 without both."""
import os
import numpy as np
from conftest import GOLDEN
import material_cases as MC
import material_seam_cases as SC
import packed_cases as KC
import points_cases as PC

ARRAYS = ("pos", "uv", "nrm", "idx_pos", "idx_uv", "idx_nrm")
PASS_GROUP = "geodec.k7b_material_table"            # the third table's pass: recorded by the calls that return materials, by no other
# the frames of check 1: the smallest shapes at which each part of the pass can go wrong (material_seam_cases has the patterns)
FRAMES = ("small_sphere_bands", "grid_checkerboard", "grid_checkerboard_retry", "sphere_pinwheel", "torus_island", "grid_stripes", "soup", "shells_split_degenerate")


def frames(names=FRAMES):
    F = {f[0]: f for f in SC.seam_frames()}
    return [F[k] for k in names]


def encode(cd, frs):
    return cd.encode_mesh_batch([dict(m, face_mat=fm) for _, m, fm, _ in frs])


def slot_files(cd):
    """small_sphere_bands with ids as the full frame, without tex-coords and without tex-coords and normals: the material in attribute-data
    slot 2, 1 and 0."""
    m, fm = SC.small_sphere_bands()
    no_uv = {k: v for k, v in m.items() if k not in ("uv", "idx_uv")}
    bare = dict(pos=m["pos"], idx_pos=m["idx_pos"])
    return cd.encode_mesh_batch([dict(f, face_mat=fm) for f in (m, no_uv, bare)])


def corner_material(d):
    """The oracle's row of the corner-form material attribute (the last decoder: GENERIC uint8, one component, dec_type 1) or None."""
    a = d.atts[-1]
    return a if (a["att_type"] == 4 and a["data_type"] == 2 and a["ncomp"] == 1 and a["dec_type"] == 1 and a["seq_type"] == 1) else None


def want_face_mat(O, data):
    d = O.drc_decode(data)
    assert d.leftover == 0
    return MC.face_values(d)[:, 0]


def same_arrays(a, b, tag):
    for k in ARRAYS:
        assert np.array_equal(np.asarray(a[k]).view(np.uint32), np.asarray(b[k]).view(np.uint32)), (tag, k)


# ---------------------------------------------------------------------------------------------- checks 1 and 2
def run_mat(O, cd, mem, files, slots=None):
    """uvol_decode_mesh_batch_mat, host and device outputs: has_mat 1, face_mat the oracle's column 0, the six arrays bit-equal to those of
    uvol_decode_mesh_batch[_dev] on the same file (and equal to the oracle's).  slots: the attribute-data slot every file must use."""
    for i, f in enumerate(files):
        d = O.drc_decode(f); a = corner_material(d)
        assert d.leftover == 0 and a is not None, i
        if slots is not None: assert a["att_data_id"] == slots[i] and d.nad == slots[i] + 1, (i, a["att_data_id"])
    want = [want_face_mat(O, f) for f in files]
    for on_device in (False, True):
        got = MC.decode_raw(cd, mem, files, on_device, True)
        ref = MC.decode_raw(cd, mem, files, on_device, False)
        for i, (g, r, w) in enumerate(zip(got, ref, want)):
            assert g["has_mat"] == 1, (i, on_device)
            assert g["n_faces"] == len(w) and np.array_equal(g["face_mat"], w), (i, on_device, int((g["face_mat"] != w).sum()))
            same_arrays(g, r, (i, on_device))
        mem.free_all()
    for f, g in zip(files, cd.decode_mesh_batch(files)):                        # the plain call against the oracle, once
        PC.check_old_decode(O, f, g)
    py = cd.decode_mesh_batch(files, materials=True)                            # the binding: no interface change
    for g, w in zip(py, want):
        assert np.array_equal(g["face_mat"], w)


def run_retry(O, cd):
    """The GD_E_WS_OVERFLOW retry covers the third table.  The decoder's compact workspace holds 1.5 x faces + 4096 entries; a checkerboard
    has 3 material vertices per face, so it overflows past 2731 faces: the 40 x 28 grid of check 1 (2074) fits, the 56 x 40 grid (4258)
    must be decoded again, alone, with worst-case sizes - seen as a second launch of the first stage of the one call."""
    fits, big = (SC.grid_checkerboard(40, 28), SC.grid_checkerboard(56, 40))
    assert MC.nfaces(fits[0]) <= 2731 < MC.nfaces(big[0])
    files = cd.encode_mesh_batch([dict(m, face_mat=fm) for m, fm in (fits, big)])
    launches = lambda: {g["name"]: g["launches"] for g in cd.profile_report()}
    cd.profile(True)
    try:
        for f, n in zip(files, (1, 2)):
            cd.profile_reset()
            g = cd.decode_mesh_batch([f], materials=True)[0]
            la = launches()
            assert la["geodec.k1_index"] == n and la[PASS_GROUP] == n, la
            assert np.array_equal(g["face_mat"], want_face_mat(O, f))
            PC.check_old_decode(O, f, g)
            cd.profile_reset()
            p = cd.decode_mesh_batch_packed([f])[0]
            assert launches()["geodec.k1_index"] == n
            KC.check_frame(packed_reference(O, f), p, "retry")
    finally:
        cd.profile(False)


# ---------------------------------------------------------------------------------------------- check 3
def packed_reference(O, data):
    """Expected packed result of one file from the oracle decoder alone.  A frame whose material is a corner attribute: the point tuple is
    (position entry, tex-coord entry, normal entry, corner material); any other frame: packed_cases.reference."""
    d = O.drc_decode(data)
    mat = corner_material(d)
    if mat is None:
        return KC.reference(O, data)
    atts = {key: d.att(name) for name, key, _ in PC.NAMES}
    present = [k for k in ("pos", "uv", "nrm") if atts[k] is not None]
    cmat = mat["vals"][:, 0][mat["corner_to_entry"]].astype(np.int64)
    keys = np.stack([atts[k]["corner_to_entry"].astype(np.int64) for k in present] + [cmat], axis=1)
    uniq, first, inv = np.unique(keys, axis=0, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")
    rank = np.empty(len(order), np.int64); rank[order] = np.arange(len(order))
    rows = dict(zip(present + ["mat"], uniq[order].T))
    n = len(order)
    rec = np.zeros(n, KC.RECORD)
    rec["pos"] = atts["pos"]["vals"][rows["pos"], :3]
    if atts["uv"] is not None: rec["uv"] = atts["uv"]["vals"][rows["uv"], :2]
    if atts["nrm"] is not None: rec["nrm"][:, :3] = np.rint(atts["nrm"]["float"][rows["nrm"]] * np.float32(127)).astype(np.int8)
    rec["material"] = rows["mat"]
    uv = atts["uv"]
    return dict(n_faces=d.nf, n_points=n, index=rank[np.asarray(inv).reshape(-1)].astype(np.uint32), records=rec, has_uv=uv is not None, has_nrm=atts["nrm"] is not None,
                has_material=True, pos_bits=atts["pos"]["qbits"], uv_bits=uv["qbits"] if uv is not None else 0,
                pos_min=np.array(atts["pos"]["minv"][:3], np.float32), pos_scale=KC.scale_of(atts["pos"]),
                uv_min=np.array(uv["minv"][:2], np.float32) if uv is not None else np.zeros(2, np.float32), uv_scale=KC.scale_of(uv) if uv is not None else np.float32(0))


def run_packed(O, cd, files, tags):
    """uvol_decode_mesh_batch_packed: index, n_points, the records and the flags are the reference's; the material at each face's first corner
    is uvol_decode_mesh_batch_mat's per-face id; n_points <= 3 x faces.  -> {tag: (packed n_points, n_points of _points)}."""
    got = cd.decode_mesh_batch_packed(files)
    facemat = cd.decode_mesh_batch(files, materials=True)
    pts = cd.decode_mesh_batch_points(files, layout="interleaved")
    out = {}
    for tag, f, g, fmat, p in zip(tags, files, got, facemat, pts):
        r = packed_reference(O, f)
        KC.check_frame(r, g, tag)
        assert g["has_material"] and g["n_points"] <= 3 * g["n_faces"], tag
        rec = np.asarray(g["records"]).view(KC.RECORD).reshape(-1)
        assert np.array_equal(rec["material"][np.asarray(g["index"])[0::3]], fmat["face_mat"]), tag
        PC.check_frame(PC.reference(O, f), p, "interleaved", tag)               # the float form does not know materials: its points are unchanged
        assert g["n_points"] >= p["n_points"], tag
        if g["n_points"] == p["n_points"]: assert np.array_equal(g["index"], p["index"]), tag      # no tuple carries two ids: the same points
        out[tag] = (g["n_points"], p["n_points"])
    return out


def run_packed_point_counts(O, cd):
    """sphere_charts: material seams coincide with tex-coord seams, no (position, tex-coord, normal) tuple carries two ids - the points are
    those of _points; torus_halves: the seam runs through tuples the float form shares - more points."""
    frs = frames(("sphere_charts", "torus_halves"))
    n = run_packed(O, cd, encode(cd, frs), [f[0] for f in frs])
    assert n["sphere_charts"][0] == n["sphere_charts"][1], n
    assert n["torus_halves"][0] > n["torus_halves"][1], n


# ---------------------------------------------------------------------------------------------- check 4
def ragged_files(cd):
    """slot 2, slot 1, slot 0, a vertex-form material file, a file without materials, the recorded 00000.drc."""
    name, m, fm, _, _ = MC.value_frames()[2]
    vertex_form = cd.encode_mesh(**m, face_mat=fm)
    bare = cd.encode_mesh(**MC.plain(MC.small_meshes()[2]))
    return slot_files(cd) + [vertex_form, bare, open(os.path.join(GOLDEN, "00000.drc"), "rb").read()]


def run_ragged(O, cd):
    """One ragged batch in one call, through _mat (host outputs) and _packed: every result equals the file decoded alone; the three frames
    without a corner material are bit-identical to what a call gives with the slot-2 / 1 / 0 files left out."""
    files = ragged_files(cd)
    for i, f in enumerate(files):
        d = O.drc_decode(f)
        assert (corner_material(d) is not None) == (i < 3) and (KC.material_attribute(d) is not None) == (i in (3, 5)), i
    def mat(fl):
        return cd.decode_mesh_batch(fl, materials=True)
    def same_mat(a, b, tag):
        same_arrays({k: (a[k] if a[k] is not None else np.zeros(0, np.uint32)) for k in ARRAYS}, {k: (b[k] if b[k] is not None else np.zeros(0, np.uint32)) for k in ARRAYS}, tag)
        assert (a["face_mat"] is None) == (b["face_mat"] is None) and (a["face_mat"] is None or np.array_equal(a["face_mat"], b["face_mat"])), tag
    def same_packed(a, b, tag):
        assert all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in KC.META + ("index", "pos_min", "pos_scale", "uv_min", "uv_scale")), tag
        assert np.array_equal(KC.raw(a["records"]), KC.raw(b["records"])), tag
    results = {}
    for name, call, same in (("mat", mat, same_mat), ("packed", cd.decode_mesh_batch_packed, same_packed)):
        batch = call(files); rest = call(files[3:]); alone = [call([f])[0] for f in files]
        for i in range(len(files)):
            same(batch[i], alone[i], (name, "alone", i))
        for i in range(3, len(files)):
            same(rest[i - 3], alone[i], (name, "without the corner-form files", i))
        results[name] = batch
    for i, f in enumerate(files):
        PC.check_old_decode(O, f, results["mat"][i])
        if i in (0, 1, 2, 3, 5): assert np.array_equal(results["mat"][i]["face_mat"], want_face_mat(O, f)), i
        else: assert results["mat"][i]["face_mat"] is None
        KC.check_frame(packed_reference(O, f), results["packed"][i], ("ragged packed", i))


# ---------------------------------------------------------------------------------------------- check 5
def run_plain_stays_plain(O, cd):
    """uvol_decode_mesh_batch and _points on a slot-2 file succeed and equal the oracle; with profiling on they record no group of the
    third table's pass, and the plain call no weld group - before and after a _mat and a _packed call on the context."""
    f = slot_files(cd)[0]
    groups = lambda: {g["name"] for g in cd.profile_report() if g["launches"] > 0}
    def plain_calls():
        cd.profile_reset()
        PC.check_old_decode(O, f, cd.decode_mesh_batch([f])[0])
        a = groups()
        assert PASS_GROUP not in a and not any("weld" in nm for nm in a) and "geodec.k8_finish" in a, a
        cd.profile_reset()
        for layout in ("planar", "interleaved"):
            PC.check_frame(PC.reference(O, f), cd.decode_mesh_batch_points([f], layout=layout)[0], layout)
        b = groups()
        assert PASS_GROUP not in b and b - a == {"geodec.k9_weld"}, (a, b)
        return a
    cd.profile(True)
    try:
        before = plain_calls()
        cd.profile_reset()
        assert np.array_equal(cd.decode_mesh_batch([f], materials=True)[0]["face_mat"], want_face_mat(O, f))
        assert groups() - before == {PASS_GROUP}, groups()                       # the _mat call: the plain call's stages and the pass
        cd.profile_reset()
        KC.check_frame(packed_reference(O, f), cd.decode_mesh_batch_packed([f])[0], "packed")
        assert PASS_GROUP in groups()
        assert plain_calls() == before
    finally:
        cd.profile(False)


# ---------------------------------------------------------------------------------------------- check 6 (host emulation only)
def corrupt_variants(O, data, seed=7):
    """Byte flips and truncations of a slot-2 file, aimed at what the pass reads: the material decoder's section (prediction bytes, symbol
    table, payload, wrap bounds), the decoder rows ahead of the attribute sections, the third seam stream - and a few anywhere."""
    d = O.drc_decode(data); a = d.atts[-1]
    rng = np.random.default_rng(seed)
    seam3 = MC.seam_pieces(data)[-1]; s0 = data.index(seam3)
    first_sec = min(x["sec_begin"] for x in d.atts)
    spots = list(range(a["sec_begin"], a["sec_end"])) + list(range(s0, s0 + len(seam3))) + list(range(first_sec - 40, first_sec))
    spots += [int(x) for x in rng.integers(11, len(data), 12)]
    out = []
    for o in spots:
        b = bytearray(data); b[o] ^= int(rng.integers(1, 256)); out.append(bytes(b))
    for cut in (a["sec_begin"], a["sec_begin"] + 3, (a["sec_begin"] + a["sec_end"]) // 2, a["sec_end"] - 1, s0 + 1, len(data) // 2):
        out.append(data[:cut])
    return out


def run_corrupt(O, cd):
    """Every call returns; the bad frame gets a status or decodes to something; the good frame beside it is unchanged."""
    good_f, bad_src = slot_files(cd)[1], slot_files(cd)[0]
    calls = (lambda fl: cd.decode_mesh_batch(fl, raise_on_error=False), lambda fl: cd.decode_mesh_batch(fl, raise_on_error=False, materials=True),
             lambda fl: cd.decode_mesh_batch_points(fl, raise_on_error=False), lambda fl: cd.decode_mesh_batch_packed(fl, raise_on_error=False))
    good = [c([good_f])[0] for c in calls]
    def same(a, b):
        assert a is not None and a.keys() == b.keys()
        for k in a:
            if a[k] is None: assert b[k] is None
            else: assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    variants = corrupt_variants(O, bad_src)
    failed = 0
    for v in variants:
        try: cd.drc_info(v); header_ok = True
        except Exception: header_ok = False                                     # (the binding sizes the plain outputs by the header: such a file never reaches that call)
        for k, (c, g) in enumerate(zip(calls, good)):
            if k < 2 and not header_ok: continue
            res = c([v, good_f])
            assert len(res) == 2
            same(res[1], g)
            failed += res[0] is None
    assert failed > 0                                                           # (some of them are refused: the statuses do travel)
    return len(variants)
