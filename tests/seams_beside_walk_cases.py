"""The batch shared by tests/test_hipemu_seams_beside_walk.py (host emulation of the kernels) and tests/test_gpu_seams_beside_walk.py
(MI355X): 19 small distinct frames - a count that is no multiple of any walker-per-wave setting - for the two forms of the group enqueue:
the lane's auxiliary stream (valence replay) joined before the record tables of the traversals (early) or behind the traversals (late).
(The files are named after the change they were written for - seam flags and attribute vertices beside the walk -, which measured
slower and was not kept; what they check holds for the enqueue that was.)"""
import ctypes as C
import numpy as np
import material_cases as MC

N_FRAMES = 19
REFUSED = 9            # index of the frame the encoder refuses (two materials meet at shared vertices: material_cases.run_refusal)


def frames():
    """19 frames: thirteen spheres of ~300 vertices with chart seams in both attributes (texture charts, creased normals), two tori, a
    positions-only frame, two open meshes with boundaries, and - in the middle - a torus whose halves carry different material ids."""
    import synth
    t = synth.torus_mesh()
    seam = np.zeros(MC.nfaces(t), np.uint8); seam[MC.nfaces(t) // 2:] = 3
    sph = synth.distinct_meshes(13, 24, 13, bases=3, charts=(3, 2))       # (each its own tessellation: the walkers of a wave diverge)
    out = sph[:9] + [dict(t, face_mat=seam)] + sph[9:] + [synth.torus_mesh(16, 8), MC.plain(t),
          dict(pos=sph[0]["pos"], idx_pos=sph[0]["idx_pos"]), synth.grid_mesh(), synth.grid_mesh(10, 7, seed=5)]
    assert len(out) == N_FRAMES and "face_mat" in out[REFUSED]
    return out


def oracle_bytes(O, f):
    return O.drc_encode(f["pos"], f["idx_pos"], f.get("uv"), f.get("idx_uv"), f.get("nrm"), f.get("idx_nrm"))


def encode_with_status(cd, fs):
    """uvol_encode_mesh_batch_mat on host frames -> (bytes per frame, status per frame)."""
    import uvol
    n = len(fs); meshes = (uvol.Mesh * n)(); keep = []; fms = []
    for i, f in enumerate(fs):
        m, k, fm = cd._mesh_host_mat(**f); meshes[i] = m; keep.append(k); fms.append(fm)
    mats = cd._mat_ptrs(fms)
    outs = (C.c_void_p * n)(); caps = (C.c_size_t * n)(); lens = (C.c_size_t * n)(); st = (C.c_int * n)(); bufs = []
    for i in range(n):
        caps[i] = cd.L.uvol_mesh_bound_mat(C.byref(meshes[i])); bufs.append(np.empty(caps[i], np.uint8)); outs[i] = bufs[i].ctypes.data
    assert cd.L.uvol_encode_mesh_batch_mat(cd.h, meshes, mats, n, 0, outs, caps, lens, st) == 0
    return [bufs[i][:lens[i]].tobytes() for i in range(n)], list(st)


def run_batch(O, cd):
    """Every good frame equals the oracle byte for byte; the refused frame keeps its status and its neighbours keep their bytes."""
    import uvol
    fs = frames()
    got, st = encode_with_status(cd, fs)
    for i, f in enumerate(fs):
        if i == REFUSED:
            assert st[i] == uvol.UVOL_E_UNSUPPORTED, st
        else:
            assert st[i] == uvol.UVOL_OK and got[i] == oracle_bytes(O, f), i
    assert "mesh %d" % REFUSED in cd.error() and "material" in cd.error()
