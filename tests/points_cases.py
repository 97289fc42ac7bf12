"""Checks of the render-ready mesh decode (uvol_decode_mesh_batch_points: one index per corner, one value record per point) shared by
tests/test_hipemu_points.py (host emulation of the kernels) and tests/test_gpu_points.py (MI355X).  Every check takes the oracle module,
a uvol.Codec and, where device memory is involved, a Mem of tests/material_cases.py.

The reference is computed here, in NumPy, from the ORACLE decoder's output and never from the library's: the tuples
(corner_to_entry of position, tex-coord, normal) are stacked, np.unique(axis=0) finds the distinct ones, and the unique rows are re-ranked
by the corner of their first appearance.  Every comparison is on the float bit patterns."""
import ctypes as C
import glob
import os
import zlib
import numpy as np
from conftest import GOLDEN, REF_OUT
import material_cases as MC

NAMES = (("position", "pos", 3), ("tex_coord", "uv", 2), ("normal", "nrm", 3))
U32 = np.uint32


def recorded_files(step=1):
    """The reference's recorded .drc files (250); step > 1: every step-th plus 00000 and 00075."""
    paths = sorted(glob.glob(os.path.join(REF_OUT, "**", "*.drc"), recursive=True))
    assert len(paths) == 250, len(paths)
    pick = [p for i, p in enumerate(paths) if i % step == 0 or os.path.basename(p) in ("00000.drc", "00075.drc")]
    return [open(p, "rb").read() for p in pick]


def reference(O, data):
    """Expected result of one file, from the oracle decoder alone."""
    d = O.drc_decode(data)
    atts = {key: d.att(name) for name, key, _ in NAMES}
    assert atts["pos"] is not None
    cols = [atts[k]["corner_to_entry"].astype(np.int64) for k in ("pos", "uv", "nrm") if atts[k] is not None]
    keys = np.stack(cols, axis=1)
    uniq, first, inv = np.unique(keys, axis=0, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")                 # unique rows in the order of their first corner
    rank = np.empty(len(order), np.int64); rank[order] = np.arange(len(order))
    rows = uniq[order]
    ref = dict(n_faces=d.nf, n_points=len(rows), index=rank[np.asarray(inv).reshape(-1)].astype(U32), has_uv=atts["uv"] is not None, has_nrm=atts["nrm"] is not None)
    col = 0
    for k in ("pos", "uv", "nrm"):
        if atts[k] is None:
            ref[k] = None; continue
        ref[k] = np.ascontiguousarray(atts[k]["float"][rows[:, col]], np.float32); col += 1
    return ref


def interleave(ref):
    """[n, 8] float32 record pos[3] nrm[3] uv[2], absent slots zero."""
    out = np.zeros((ref["n_points"], 8), np.float32)
    out[:, 0:3] = ref["pos"]
    if ref["nrm"] is not None: out[:, 3:6] = ref["nrm"]
    if ref["uv"] is not None: out[:, 6:8] = ref["uv"]
    return out


def same_bits(a, b):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(U32), b.view(U32))


def check_frame(ref, got, layout, tag=""):
    assert got is not None, tag
    assert (got["n_faces"], got["n_points"], bool(got["has_uv"]), bool(got["has_nrm"])) == (ref["n_faces"], ref["n_points"], ref["has_uv"], ref["has_nrm"]), (tag, got["n_faces"], got["n_points"], ref["n_points"])
    assert np.array_equal(np.asarray(got["index"]), ref["index"]), tag
    if layout == "interleaved":
        assert same_bits(got["points"], interleave(ref)), tag
    else:
        for k in ("pos", "uv", "nrm"):
            if ref[k] is None: assert got[k] is None, (tag, k)
            else: assert same_bits(got[k], ref[k]), (tag, k)


def check_renderer_invariant(old, got, layout, tag=""):
    """Without the reference: de-indexing the welded buffers equals de-indexing the existing decode's three streams, corner for corner;
    every point is referenced; index is first-appearance ordered (each new id is one more than the largest so far)."""
    idx = np.asarray(got["index"]).astype(np.int64)
    if layout == "interleaved":
        P = got["points"]; w = dict(pos=P[:, 0:3], nrm=P[:, 3:6], uv=P[:, 6:8])
    else:
        w = got
    for k in ("pos", "uv", "nrm"):
        if old[k] is None:
            if layout == "interleaved": assert not np.any(np.ascontiguousarray(w[k]).view(U32)), (tag, k)      # absent slot: zeros
            continue
        assert same_bits(np.ascontiguousarray(w[k])[idx], old[k][old["idx_" + k].astype(np.int64)]), (tag, k)
    n = got["n_points"]
    assert len(np.unique(idx)) == n and idx.min() == 0 and idx.max() == n - 1, tag
    prev = np.concatenate([[-1], np.maximum.accumulate(idx)[:-1]])
    assert np.all(idx <= prev + 1), tag


def check_old_decode(O, data, got):
    """uvol_decode_mesh_batch against the oracle, as the existing tests compare it."""
    want = O.drc_decode(data)
    assert got["n_faces"] == want.nf
    for name, key, _ in NAMES:
        a = want.att(name)
        if a is None:
            assert got[key] is None; continue
        assert same_bits(got[key], a["float"]), name
        assert np.array_equal(got["idx_" + key], a["corner_to_entry"].astype(U32)), name


# ---------------------------------------------------------------------------------------------- check 1
def run_recorded(O, cd, files, invariant_on=None):
    """Recorded files, both layouts, one call per layout; the reference on every file and the renderer's invariant (against the existing
    decode of the same files) on the frames `invariant_on` lists (default: all)."""
    refs = [reference(O, f) for f in files]
    inv = list(range(len(files))) if invariant_on is None else list(invariant_on)
    old = dict(zip(inv, cd.decode_mesh_batch([files[i] for i in inv])))
    for layout in ("planar", "interleaved"):
        got = cd.decode_mesh_batch_points(files, layout=layout)
        assert len(got) == len(files)
        for i, (r, g) in enumerate(zip(refs, got)):
            check_frame(r, g, layout, (layout, i))
            if i in old: check_renderer_invariant(old[i], g, layout, (layout, i))
    return len(files)


# ---------------------------------------------------------------------------------------------- check 2
def subset_streams(cd, cd0):
    """(name, .drc) of the attribute subsets and tool sets, encoded by the library: positions only, positions + uv, all three with seams
    (a sphere with charts), a `-cl 0` (sequential) stream of each of the last two."""
    import synth
    t, s, g = MC.small_meshes()
    out = [("pos_only", cd.encode_mesh(pos=t["pos"], idx_pos=t["idx_pos"])),
           ("pos_uv", cd.encode_mesh(pos=t["pos"], idx_pos=t["idx_pos"], uv=t["uv"], idx_uv=t["idx_uv"])),
           ("pos_nrm", cd.encode_mesh(pos=g["pos"], idx_pos=g["idx_pos"], nrm=g["nrm"], idx_nrm=g["idx_nrm"])),
           ("all_three_seams", cd.encode_mesh(**MC.plain(s))),
           ("all_three_grid_holes", cd.encode_mesh(**MC.plain(g))),
           ("soup", cd.encode_mesh(**MC.plain(synth.random_soup_mesh(5)))),
           ("cl0_all_three", cd0.encode_mesh(**MC.plain(s))),
           ("cl0_pos_uv", cd0.encode_mesh(pos=t["pos"], idx_pos=t["idx_pos"], uv=t["uv"], idx_uv=t["idx_uv"]))]
    return out


def run_subsets(O, cd, cd0):
    streams = subset_streams(cd, cd0)
    files = [f for _, f in streams]
    want_has = dict(pos_only=(False, False), pos_uv=(True, False), pos_nrm=(False, True), all_three_seams=(True, True), all_three_grid_holes=(True, True),
                    soup=(True, True), cl0_all_three=(True, True), cl0_pos_uv=(True, False))
    assert O.drc_decode(files[-2]).method == 0 and O.drc_decode(files[3]).method == 1          # the sequential stream is one
    refs = [reference(O, f) for f in files]
    old = cd.decode_mesh_batch(files)
    for layout in ("planar", "interleaved"):
        got = cd.decode_mesh_batch_points(files, layout=layout)
        for (name, _), r, g, o in zip(streams, refs, got, old):
            assert (bool(g["has_uv"]), bool(g["has_nrm"])) == want_has[name], name
            check_frame(r, g, layout, (layout, name))
            check_renderer_invariant(o, g, layout, (layout, name))
            if layout == "interleaved":
                if not g["has_nrm"]: assert not np.any(g["points"][:, 3:6].view(U32)), name
                if not g["has_uv"]: assert not np.any(g["points"][:, 6:8].view(U32)), name
    # seams make points: the charted sphere has more points than position entries, a frame without uv / normals exactly as many
    assert refs[3]["n_points"] > len(old[3]["pos"]) and refs[0]["n_points"] == len(old[0]["pos"])
    return files


# ---------------------------------------------------------------------------------------------- check 3
def run_ragged(O, cd, cd0):
    """Files of different sizes, a truncated and a foreign file, a frame with cap_points one below its count, a frame whose index array is
    too small: those fail alone with the documented codes, n_points of the short frame is the needed count, the others are bit-exact."""
    import uvol
    good = [f for _, f in subset_streams(cd, cd0)] + [open(os.path.join(GOLDEN, "00000.drc"), "rb").read()]
    trunc = good[3][:len(good[3]) * 2 // 3]; foreign = b"OBJ? no: not a Draco file at all " * 8
    files = [good[0], trunc, good[3], foreign, good[8], good[4], good[6], good[1], good[5]]
    SHORT, FEW_FACES, TRUNC, FOREIGN = 5, 7, 1, 3
    refs = {i: reference(O, f) for i, f in enumerate(files) if i not in (TRUNC, FOREIGN)}
    for layout in ("planar", "interleaved"):
        metas = (uvol.DecodedPoints * len(files))()
        for i, f in enumerate(files):
            if i == FOREIGN:
                metas[i].cap_faces = 100; metas[i].cap_points = 300; continue
            nf, mv = cd.drc_info(f); metas[i].cap_faces = nf; metas[i].cap_points = mv
        metas[SHORT].cap_points = refs[SHORT]["n_points"] - 1
        metas[FEW_FACES].cap_faces = refs[FEW_FACES]["n_faces"] - 1
        st = []
        got = cd.decode_mesh_batch_points(files, layout=layout, raise_on_error=False, metas=metas, status_out=st)
        assert st[TRUNC] == uvol.UVOL_E_ENCODE and st[FOREIGN] == uvol.UVOL_E_INVALID and st[SHORT] == uvol.UVOL_E_NOSPACE and st[FEW_FACES] == uvol.UVOL_E_NOSPACE, st
        assert metas[SHORT].n_points == refs[SHORT]["n_points"] and metas[FEW_FACES].n_faces == refs[FEW_FACES]["n_faces"]
        for i in range(len(files)):
            if i in (TRUNC, FOREIGN, SHORT, FEW_FACES):
                assert got[i] is None; continue
            assert st[i] == 0
            check_frame(refs[i], got[i], layout, (layout, i))
        # the capacity that is exactly enough is enough
        two = (uvol.DecodedPoints * 2)()
        two[0].cap_faces = metas[SHORT].cap_faces; two[0].cap_points = refs[SHORT]["n_points"]; two[1].cap_faces = refs[FEW_FACES]["n_faces"]; two[1].cap_points = metas[FEW_FACES].cap_points
        got = cd.decode_mesh_batch_points([files[SHORT], files[FEW_FACES]], layout=layout, metas=two)
        check_frame(refs[SHORT], got[0], layout); check_frame(refs[FEW_FACES], got[1], layout)
    # without a status array the call reports the worst frame; a lone good frame is UVOL_OK
    n = 2; fl = [files[0], foreign]
    metas = (uvol.DecodedPoints * n)(); keep = []
    for i in range(n):
        metas[i].cap_faces = 4096; metas[i].cap_points = 3 * 4096
        a = [np.zeros(3 * 4096 * w, np.float32) for w in (3, 2, 3)] + [np.zeros(3 * 4096, U32)]; keep.append(a)
        metas[i].pos, metas[i].uv, metas[i].nrm, metas[i].index = (x.ctypes.data for x in a)
    fp = (C.c_char_p * n)(*fl); ln = (C.c_size_t * n)(*[len(f) for f in fl])
    assert cd.L.uvol_decode_mesh_batch_points(cd.h, fp, ln, n, 0, metas, None) == uvol.UVOL_E_INVALID
    assert cd.L.uvol_decode_mesh_batch_points(cd.h, fp, ln, 1, 0, metas, None) == uvol.UVOL_OK and metas[0].n_points == refs[0]["n_points"]
    metas[0].layout = 7
    assert cd.L.uvol_decode_mesh_batch_points(cd.h, fp, ln, 1, 0, metas, None) == uvol.UVOL_E_INVALID


def disk_mesh(k):
    """k triangles around one centre vertex: the centre's position entry is shared by k corners."""
    a = 2 * np.pi * np.arange(k) / k
    pos = np.concatenate([[[0, 0, 0]], np.stack([np.cos(a), np.sin(a), 0.1 * np.sin(3 * a)], axis=1)]).astype(np.float32)
    ring = 1 + np.arange(k)
    idx = np.stack([np.zeros(k, np.int64), ring, 1 + (np.arange(k) + 1) % k], axis=1).reshape(-1).astype(U32)
    return dict(pos=pos, idx_pos=idx)


def run_long_fan(O, cd, cd0):
    """The documented limit of the weld: a position entry shared by more than 4096 corners (a sequential, `-cl 0`, stream of a disk of
    4200 triangles around one vertex) fails ALONE with UVOL_E_UNSUPPORTED on this entry point, while uvol_decode_mesh_batch still decodes
    the file; a disk of exactly 4096 triangles, and the neighbours in the batch, come out bit-exact."""
    import uvol
    at, over = cd0.encode_mesh(**disk_mesh(4096)), cd0.encode_mesh(**disk_mesh(4200))
    assert O.drc_decode(over).method == 0
    for f in (at, over):
        d = O.drc_decode(f); cnt = np.bincount(d.att("position")["corner_to_entry"])
        assert cnt.max() == d.nf and d.nf in (4096, 4200)                      # the encoder kept the fan whole
    good = cd.encode_mesh(**MC.plain(MC.small_meshes()[1]))
    files = [good, over, at, good]
    for f, g in zip(files, cd.decode_mesh_batch(files)):
        check_old_decode(O, f, g)
    refs = [reference(O, f) for f in files]
    for layout in ("planar", "interleaved"):
        st = []
        got = cd.decode_mesh_batch_points(files, layout=layout, raise_on_error=False, status_out=st)
        assert st == [0, uvol.UVOL_E_UNSUPPORTED, 0, 0], st
        assert got[1] is None
        for i in (0, 2, 3):
            check_frame(refs[i], got[i], layout, (layout, i))


# ---------------------------------------------------------------------------------------------- check 4
def decode_dev(cd, mem, files, layout, caps=None):
    """Device outputs through `mem` -> (statuses, metas, list of host copies as decode_mesh_batch_points returns them)."""
    import uvol
    n = len(files); metas = (uvol.DecodedPoints * n)(); ptr = []
    for i, f in enumerate(files):
        nf, mv = cd.drc_info(f) if caps is None else caps[i]
        metas[i].cap_faces = nf; metas[i].cap_points = mv
        row = dict(index=mem.alloc(12 * nf))
        if layout == "interleaved":
            row["pos"] = mem.alloc(32 * mv); metas[i].pos = row["pos"]
        else:
            row.update(pos=mem.alloc(12 * mv), uv=mem.alloc(8 * mv), nrm=mem.alloc(12 * mv))
            metas[i].pos, metas[i].uv, metas[i].nrm = row["pos"], row["uv"], row["nrm"]
        metas[i].index = row["index"]; ptr.append(row)
    st = cd.decode_mesh_batch_points(files, layout=layout, on_device=True, metas=metas)
    out = []
    for i in range(n):
        m = metas[i]
        if st[i] != 0:
            out.append(None); continue
        r = dict(index=mem.to_host(ptr[i]["index"], U32, 3 * m.n_faces), n_faces=m.n_faces, n_points=m.n_points, has_uv=bool(m.has_uv), has_nrm=bool(m.has_nrm))
        if layout == "interleaved":
            r["points"] = mem.to_host(ptr[i]["pos"], np.float32, 8 * m.n_points).reshape(-1, 8)
        else:
            r["pos"] = mem.to_host(ptr[i]["pos"], np.float32, 3 * m.n_points).reshape(-1, 3)
            r["uv"] = mem.to_host(ptr[i]["uv"], np.float32, 2 * m.n_points).reshape(-1, 2) if m.has_uv else None
            r["nrm"] = mem.to_host(ptr[i]["nrm"], np.float32, 3 * m.n_points).reshape(-1, 3) if m.has_nrm else None
        out.append(r)
    return st, metas, out, ptr


def run_memory_forms(O, cd, cd0, mem, lib_path=None):
    """Device outputs, pageable host outputs and outputs in a PinnedArena: all the reference's."""
    import uvol
    files = [f for _, f in subset_streams(cd, cd0)] + [open(os.path.join(GOLDEN, "00075.drc"), "rb").read()]
    refs = [reference(O, f) for f in files]
    for layout in ("planar", "interleaved"):
        st, _, dev, _ = decode_dev(cd, mem, files, layout)
        assert st == [0] * len(files)
        host = cd.decode_mesh_batch_points(files, layout=layout)
        ar = uvol.PinnedArena(cd.points_arena_bytes(files), lib_path=lib_path)
        try:
            pinned = cd.decode_mesh_batch_points(files, layout=layout, arena=ar)
            for i, r in enumerate(refs):
                for form, got in (("device", dev), ("host", host), ("pinned", pinned)):
                    check_frame(r, got[i], layout, (layout, form, i))
        finally:
            del pinned; ar.close()
        mem.free_all()
    # a short frame among device outputs: nothing of it is written, its neighbours are
    caps = [cd.drc_info(f) for f in files[:3]]; caps[1] = (caps[1][0], refs[1]["n_points"] - 1)
    st, metas, dev, ptr = decode_dev(cd, mem, files[:3], "planar", caps)
    assert st == [0, uvol.UVOL_E_NOSPACE, 0] and metas[1].n_points == refs[1]["n_points"]
    check_frame(refs[0], dev[0], "planar"); check_frame(refs[2], dev[2], "planar")
    mem.free_all()


# ---------------------------------------------------------------------------------------------- check 5
def run_round_trip(O, cd, mem=None):
    """The planar output of a recorded file re-encoded with ONE index stream (idx_uv and idx_nrm alias idx_pos) - from device memory with
    uvol_encode_mesh_batch_dev when `mem` is given, else the host form - and decoded by the oracle: same face count, and every decoded
    position within one step of the second quantiser, range / (2^qp - 1), of the position the welded buffers hold for the same face (each
    coordinate moves at most half a step when it is re-quantised and half a step when it is read back).  Faces are matched by their
    de-indexed positions on the second quantiser's integer grid (corners rotated so that the smallest comes first).

    Face count: the recorded files hold position entries whose de-quantised values are bit-equal (00075: 27865 entries, 27289 distinct
    values; 00000: 26145 / 25742), and 1152 (806) of their faces have two corners on one such value.  The encoder merges bit-equal values
    and drops the faces that become degenerate, as stock draco_encoder does, so the re-encoded file holds n_faces minus exactly those
    faces - 54586 of 55738 for 00075 - and not n_faces: the check counts them from the welded buffers and asks for that number, and every
    other face must come back."""
    import uvol
    data = open(os.path.join(GOLDEN, "00075.drc"), "rb").read()
    if mem is None:
        g = cd.decode_mesh_batch_points([data])[0]
        re = cd.encode_mesh(pos=g["pos"], idx_pos=g["index"], uv=g["uv"], idx_uv=g["index"], nrm=g["nrm"], idx_nrm=g["index"])
    else:
        st, metas, dev, ptr = decode_dev(cd, mem, [data], "planar")
        assert st == [0]; g = dev[0]; m = metas[0]
        ms = (uvol.Mesh * 1)()
        ms[0].pos, ms[0].n_pos, ms[0].uv, ms[0].n_uv, ms[0].nrm, ms[0].n_nrm = ptr[0]["pos"], m.n_points, ptr[0]["uv"], m.n_points, ptr[0]["nrm"], m.n_points
        ms[0].idx_pos = ms[0].idx_uv = ms[0].idx_nrm = ptr[0]["index"]; ms[0].n_faces = m.n_faces
        re = bytes(cd.encode_mesh_batch_dev(ms)[0])
        mem.free_all()
    assert g["has_uv"] and g["has_nrm"]
    d = O.drc_decode(re)
    pa = d.att("position"); step = float(pa["range"]) / ((1 << pa["qbits"]) - 1)
    A = g["pos"][np.asarray(g["index"]).astype(np.int64)].reshape(-1, 3, 3)                          # welded buffers, face by face
    bits = np.ascontiguousarray(A).view(U32)
    degenerate = (bits[:, 0] == bits[:, 1]).all(1) | (bits[:, 1] == bits[:, 2]).all(1) | (bits[:, 0] == bits[:, 2]).all(1)
    print("round trip: %d faces decoded, %d welded of which %d have two corners on one position value" % (d.nf, g["n_faces"], int(degenerate.sum())))
    assert d.leftover == 0 and d.nf == g["n_faces"] - int(degenerate.sum())
    A = A[~degenerate]
    B = pa["float"][pa["corner_to_entry"]].reshape(-1, 3, 3)                                         # the oracle's decode of the re-encoded file
    qa = np.rint((A.astype(np.float64) - np.array(pa["minv"][:3], np.float64)) / step).astype(np.int64)
    qb = pa["vals"][pa["corner_to_entry"]].reshape(-1, 3, 3).astype(np.int64)

    def canon(q, x):
        code = (q[..., 0] << 42) | (q[..., 1] << 21) | q[..., 2]                                     # qp <= 20 bits per coordinate
        r = np.argmin(code, axis=1); rot = (r[:, None] + np.arange(3)[None, :]) % 3
        q = np.take_along_axis(q, rot[:, :, None], axis=1); x = np.take_along_axis(x, rot[:, :, None], axis=1)
        order = np.lexsort(q.reshape(len(q), 9).T[::-1])
        return q[order], x[order]
    qa, A = canon(qa, A); qb, B = canon(qb, B)
    assert np.array_equal(qa, qb)                                                                    # the same faces, as multisets
    dist = np.sqrt(((A.astype(np.float64) - B.astype(np.float64)) ** 2).sum(axis=2))
    print("round trip: %d faces, step %.6g, largest distance %.6g" % (d.nf, step, dist.max()))
    assert dist.max() <= step, (dist.max(), step)


# ---------------------------------------------------------------------------------------------- check 6
def run_existing_untouched(O, cd, files):
    """uvol_decode_mesh_batch returns what it returned (the oracle's decode), before and after a call of the new entry point, and records
    no kernel group of the weld; the new entry point records exactly one more."""
    groups = lambda: {g["name"] for g in cd.profile_report() if g["launches"] > 0}
    cd.profile(True); cd.profile_reset()
    try:
        for f, g in zip(files, cd.decode_mesh_batch(files)):
            check_old_decode(O, f, g)
        MC.decode_raw(cd, MC.HostMem(), files[:2], False, True)                                       # the _mat form (host outputs)
        before = groups()
        assert "geodec.k8_finish" in before and not any("weld" in nm for nm in before), before
        cd.decode_mesh_batch_points(files)
        after = groups()
        assert after - before == {"geodec.k9_weld"}, after - before
        cd.profile_reset()
        for f, g in zip(files, cd.decode_mesh_batch(files)):                                        # ... and again after the weld has used the workspace
            check_old_decode(O, f, g)
        assert groups() == before
    finally:
        cd.profile(False)


def index_crc(index):
    return zlib.crc32(np.ascontiguousarray(index, U32).tobytes())
