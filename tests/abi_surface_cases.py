"""The conventions around the C ABI that every entry point of a family shares - groups of max_batch, frames that fail in their own slot,
what is refused before any work, which output fields a failed frame keeps, the texts of uvol_last_error - pinned through the binding and
through ctypes, on the smallest inputs that reach every branch: meshes of a few dozen faces, two 8 x 8 layers per texture segment, and a
second codec with max_batch = 2.  Shared by tests/test_hipemu_abi_surface.py (host emulation of the kernels) and
tests/test_gpu_abi_surface.py (MI355X).  Every check takes `make`, which opens a uvol.Codec with the given parameters on the library under
test, and, where device memory is involved, a Mem of tests/material_cases.py.

Nothing here judges the codecs' bytes against the oracle (the other suites do): every expected value is another route through the same
library - a codec whose max_batch holds the whole call, a call that holds only the good frames, the sibling entry point."""
import ctypes as C
import numpy as np
import pytest

U8 = np.uint8
W = H = 8
NL = 2


def meshes5():
    """Five small frames (12 to 40 faces) with uv and normals, each with its own connectivity."""
    import synth
    return [synth.sphere_mesh(6, 4, charts=(2, 2)), synth.grid_mesh(5, 4), synth.torus_mesh(5, 4), synth.sphere_mesh(5, 5, charts=(1, 1)), synth.grid_mesh(4, 4, holes=False)]


def plain(m):
    return {k: m.get(k) for k in ("pos", "idx_pos", "uv", "idx_uv", "nrm", "idx_nrm")}


def nfaces(m):
    return len(m["idx_pos"]) // 3


def with_ids(frames):
    """Frame i with material id i + 1 on every face."""
    return [dict(plain(m), face_mat=np.full(nfaces(m), i + 1, U8)) for i, m in enumerate(frames)]


def same_result(a, b, tag=""):
    """Two results of the binding's decode methods (dicts of arrays, counts and flags, or None) are equal."""
    assert (a is None) == (b is None), tag
    if a is None:
        return
    assert a.keys() == b.keys(), tag
    for k in a:
        x, y = a[k], b[k]
        if x is None or y is None:
            assert x is None and y is None, (tag, k)
        elif isinstance(x, np.ndarray):
            assert x.shape == y.shape and x.tobytes() == y.tobytes(), (tag, k)
        else:
            assert x == y, (tag, k, x, y)


def files_arg(files):
    n = len(files)
    return (C.c_char_p * n)(*files), (C.c_size_t * n)(*[len(f) for f in files])


def tex_segments():
    import synth
    return [synth.texture_sequence(NL, size=W, seed=1), synth.texture_sequence(NL, size=W, seed=2)]


# ---------------------------------------------------------------------------------------------- groups of max_batch
def run_group_loop(make):
    """Five frames on a max_batch = 2 codec (groups of 2 + 2 + 1) equal those of a codec whose max_batch holds all five: encode (plain,
    views, material ids), decode (plain, views, materials).  An undecodable frame in the middle fails alone."""
    cd2, cd8 = make(max_batch=2), make(max_batch=8)
    try:
        frames = [plain(m) for m in meshes5()]; framesm = with_ids(meshes5())
        want = cd8.encode_mesh_batch(frames)
        assert len(want) == 5 and all(want) and len(set(want)) == 5
        assert cd2.encode_mesh_batch(frames) == want
        assert [bytes(v) for v in cd2.encode_mesh_batch(frames, views=True)] == want
        files = cd8.encode_mesh_batch(framesm)
        assert cd2.encode_mesh_batch(framesm) == files and all(a != b for a, b in zip(files, want))
        for kw in (dict(), dict(views=True), dict(materials=True)):
            a = cd2.decode_mesh_batch(files, **kw); b = cd8.decode_mesh_batch(files, **kw)
            assert len(a) == len(b) == 5
            for i in range(5):
                assert a[i]["n_faces"] == nfaces(frames[i])
                same_result(a[i], b[i], (kw, i))
        assert [int(r["face_mat"][0]) for r in b] == [1, 2, 3, 4, 5]
        bad = list(files); bad[2] = files[2][:len(files[2]) * 2 // 3]          # truncated: the header still reads, the payload does not
        for kw in (dict(), dict(materials=True)):
            a = cd2.decode_mesh_batch(bad, raise_on_error=False, **kw)
            assert a[2] is None
            for i in (0, 1, 3, 4):
                same_result(a[i], b[i] if kw else {k: v for k, v in b[i].items() if k != "face_mat"}, ("bad", kw, i))
            with pytest.raises(Exception, match="frame 2 failed"):
                cd2.decode_mesh_batch(bad, **kw)
    finally:
        cd2.close(); cd8.close()


# ---------------------------------------------------------------------------------------------- points and packed
POINT_OUT = ("n_faces", "n_points", "has_uv", "has_nrm")
PACKED_OUT = POINT_OUT + ("has_material", "pos_bits", "uv_bits", "pos_scale", "uv_scale")


def _form(uvol, form):
    """(struct, output fields, layout or None) of 'planar' / 'interleaved' / 'packed'."""
    if form == "packed":
        return uvol.PackedPoints, PACKED_OUT, None
    return uvol.DecodedPoints, POINT_OUT, {"planar": uvol.UVOL_POINTS_PLANAR, "interleaved": uvol.UVOL_POINTS_INTERLEAVED}[form]


def _metas(cd, uvol, form, files, short=None, arrays=False):
    """The caller's metas: capacities by uvol_drc_info (a foreign file: 100 / 300), frame `short` one face short, every output field
    preset to a non-zero value.  arrays=True: host output arrays are attached (for a call through ctypes) -> (metas, arrays)."""
    S, out, lay = _form(uvol, form)
    n = len(files); metas = (S * n)(); keep = []
    for i, f in enumerate(files):
        m = metas[i]
        try:
            nf, mv = cd.drc_info(f)
        except uvol.UvolError:
            nf, mv = 100, 300
        m.cap_faces = nf - 1 if i == short else nf; m.cap_points = mv
        for k in out:
            setattr(m, k, 7)
        if form == "packed":
            m.pos_min[:] = [7.0] * 3; m.uv_min[:] = [7.0] * 2
        else:
            m.layout = lay
        if arrays:
            a = dict(index=np.zeros(3 * max(1, nf), np.uint32), val=np.zeros((max(1, mv), 8), np.float32), uv=np.zeros((max(1, mv), 2), np.float32), nrm=np.zeros((max(1, mv), 3), np.float32))
            keep.append(a); m.index = a["index"].ctypes.data
            if form == "packed":
                m.records = a["val"].ctypes.data
            else:
                m.pos = a["val"].ctypes.data
                if form == "planar":
                    m.uv = a["uv"].ctypes.data; m.nrm = a["nrm"].ctypes.data
    return metas, keep


def _decode(cd, form, files, **kw):
    if form == "packed":
        return cd.decode_mesh_batch_packed(files, **kw)
    return cd.decode_mesh_batch_points(files, layout=form, **kw)


def _failed_fields_zero(m, form, out, but=()):
    for k in out:
        if k not in but:
            assert getattr(m, k) == 0, (form, k, getattr(m, k))
    if form == "packed":
        assert list(m.pos_min) == [0.0] * 3 and list(m.uv_min) == [0.0] * 2, form


def run_points_packed(make):
    """Five files on the max_batch = 2 codec, index 1 foreign, index 3 with cap_faces one too small: statuses [OK, E_INVALID, OK,
    E_NOSPACE, OK], n_faces of frame 3 the needed count, every other output field of the failed frames zero, frames 0 / 2 / 4 byte-equal
    to a call that holds only them.  With status = NULL the call returns the LAST failing frame's code."""
    import uvol
    cd = make(max_batch=2)
    try:
        good = cd.encode_mesh_batch(with_ids(meshes5()))
        foreign = np.random.default_rng(5).integers(0, 256, 200, dtype=U8).tobytes()
        files = [good[0], foreign, good[2], good[3], good[4]]
        need = nfaces(meshes5()[3])
        for form in ("planar", "interleaved", "packed"):
            S, out, lay = _form(uvol, form)
            metas, _ = _metas(cd, uvol, form, files, short=3)
            st = []
            got = _decode(cd, form, files, raise_on_error=False, metas=metas, status_out=st)
            assert st == [uvol.UVOL_OK, uvol.UVOL_E_INVALID, uvol.UVOL_OK, uvol.UVOL_E_NOSPACE, uvol.UVOL_OK], (form, st)
            assert got[1] is None and got[3] is None
            assert metas[3].n_faces == need, form
            _failed_fields_zero(metas[1], form, out); _failed_fields_zero(metas[3], form, out, but=("n_faces",))
            only = _decode(cd, form, [files[0], files[2], files[4]])
            for k, i in enumerate((0, 2, 4)):
                assert got[i]["n_faces"] == nfaces(meshes5()[i])
                same_result(got[i], only[k], (form, i))
            with pytest.raises(uvol.UvolError, match="frame 1 failed status=-1"):
                _decode(cd, form, files)
            # status = NULL through ctypes: the last failing frame's code, the same fields
            metas, keep = _metas(cd, uvol, form, files, short=3, arrays=True)
            fp, ln = files_arg(files)
            fn = cd.L.uvol_decode_mesh_batch_packed if form == "packed" else cd.L.uvol_decode_mesh_batch_points
            assert fn(cd.h, fp, ln, 5, 0, metas, None) == uvol.UVOL_E_NOSPACE, form
            assert cd.error() == "frame 3: %d faces, capacity %d" % (need, need - 1), cd.error()
            assert metas[3].n_faces == need and [metas[i].n_faces for i in (0, 2, 4)] == [nfaces(meshes5()[i]) for i in (0, 2, 4)]
            _failed_fields_zero(metas[1], form, out); _failed_fields_zero(metas[3], form, out, but=("n_faces",))
            for k, i in enumerate((0, 2, 4)):
                assert np.array_equal(keep[i]["index"][:3 * metas[i].n_faces], only[k]["index"]), (form, i)
            fp2, ln2 = files_arg([files[0], foreign]); m2, keep2 = _metas(cd, uvol, form, [files[0], foreign], arrays=True)
            assert fn(cd.h, fp2, ln2, 2, 0, m2, None) == uvol.UVOL_E_INVALID and cd.error() == "frame 1: not a Draco 2.2 mesh"
            assert fn(cd.h, fp2, ln2, 1, 0, m2, None) == uvol.UVOL_OK
    finally:
        cd.close()


def run_rejected_before_work(make):
    """An unknown points layout and a misaligned device pointer (an integer address that is never dereferenced) fail the whole call with
    UVOL_E_INVALID and the message of the entry point; statuses and output fields keep what the caller put there."""
    import uvol
    cd = make(max_batch=2)
    try:
        files = cd.encode_mesh_batch([plain(m) for m in meshes5()[:3]]); fp, ln = files_arg(files); n = len(files)

        def refused(fn, form, on_device, text, edit):
            metas, _ = _metas(cd, uvol, form, files); edit(metas)
            st = (C.c_int * n)(*([77] * n))
            assert fn(cd.h, fp, ln, n, on_device, metas, st) == uvol.UVOL_E_INVALID, text
            assert cd.error() == text, cd.error()
            assert list(st) == [77] * n and all(m.n_faces == 7 and m.n_points == 7 for m in metas), text

        def layout9(ms): ms[1].layout = 9
        refused(cd.L.uvol_decode_mesh_batch_points, "planar", 0, "frame 1: unknown point layout 9", layout9)
        refused(cd.L.uvol_decode_mesh_batch_points, "planar", 1, "frame 1: unknown point layout 9", layout9)

        def pos8(ms):
            for i, m in enumerate(ms): m.pos = 0x10000 + (8 if i == 2 else 0); m.index = 0x20000
        refused(cd.L.uvol_decode_mesh_batch_points, "interleaved", 1, "frame 2: the interleaved device buffer must be 16-byte aligned", pos8)

        def rec4(ms):
            for i, m in enumerate(ms): m.records = 0x10000 + (4 if i == 1 else 0); m.index = 0x20000
        refused(cd.L.uvol_decode_mesh_batch_packed, "packed", 1, "frame 1: the device records buffer must be 16-byte aligned", rec4)
    finally:
        cd.close()


# ---------------------------------------------------------------------------------------------- decode and transcode entry points
ASTC_OF_ETC1S = "ASTC 4x4 is the transcode target of UASTC sources (KTX2Loader.js:591-600); this file is ETC1S"
ENTRY = (("rgba32", "decode_texture_segments", "uvol_decode_texture_segments"), ("etc1", "transcode_texture_segments_etc1", "uvol_transcode_texture_segments_etc1"),
         ("bc7", "transcode_texture_segments_bc7", "uvol_transcode_texture_segments_bc7"), ("etc2_rgba", "transcode_texture_segments_etc2_rgba", "uvol_transcode_texture_segments_etc2_rgba"),
         ("astc", "transcode_texture_segments_astc", "uvol_transcode_texture_segments_astc"))


def run_decode_entries(make, mem):
    """The two decode and four single-target transcode entry points on one ETC1S and one UASTC file of two 8 x 8 layers: each equals
    uvol_transcode_texture_segments_st with that target; ASTC of an ETC1S file is UVOL_E_UNSUPPORTED with its message; n_segments = 0
    and a NULL array are UVOL_E_INVALID."""
    import uvol
    cd, cu = make(), make(uastc=1)
    try:
        seg = tex_segments()[0]
        srcs = dict(etc1s=cd.encode_texture_segment(seg), uastc=cu.encode_texture_segment(seg))
        assert cd.ktx2_info(srcs["etc1s"]) == (W, H, NL) and cd.ktx2_info(srcs["uastc"]) == (W, H, NL)
        for kind, f in srcs.items():
            for target, method, sym in ENTRY:
                want, st = cd.transcode_texture_segments_status([f, f], target=target)
                fn = getattr(cd.L, sym)
                unit = cd.TARGETS[target][1]; cap = 4 * unit if cd.TARGETS[target][2] else W * H * 4
                out = np.zeros((2, NL, cap), U8); ptrs = (C.c_void_p * (2 * NL))(*[out[s][l].ctypes.data for s in range(2) for l in range(NL)])
                fp, ln = files_arg([f, f]); tail = () if target == "rgba32" else (0,)
                if kind == "etc1s" and target == "astc":
                    assert st == [uvol.UVOL_E_UNSUPPORTED] * 2 and want == [None, None]
                    with pytest.raises(uvol.UvolError) as e:
                        getattr(cd, method)([f, f])
                    assert str(e.value) == "%s rc=%d: %s" % (method, uvol.UVOL_E_UNSUPPORTED, ASTC_OF_ETC1S)
                    assert fn(cd.h, fp, ln, 2, ptrs, cap, *tail) == uvol.UVOL_E_UNSUPPORTED and cd.error() == ASTC_OF_ETC1S
                else:
                    assert st == [0, 0]
                    got = getattr(cd, method)([f, f])
                    assert len(got) == 2 and all(g.shape == w.shape and g.tobytes() == w.tobytes() for g, w in zip(got, want)), (kind, target)
                    assert fn(cd.h, fp, ln, 2, ptrs, cap, *tail) == uvol.UVOL_OK
                    assert all(out[s].tobytes() == want[s].tobytes() for s in range(2)), (kind, target)
                assert fn(cd.h, fp, ln, 0, ptrs, cap, *tail) == uvol.UVOL_E_INVALID
                assert fn(cd.h, None, ln, 2, ptrs, cap, *tail) == uvol.UVOL_E_INVALID and fn(cd.h, fp, None, 2, ptrs, cap, *tail) == uvol.UVOL_E_INVALID
                assert fn(cd.h, fp, ln, 2, None, cap, *tail) == uvol.UVOL_E_INVALID and fn(None, fp, ln, 2, ptrs, cap, *tail) == uvol.UVOL_E_INVALID
            # the device forms: layers in device memory
            want, _ = cd.transcode_texture_segments_status([f], target="rgba32")
            dev = [mem.alloc(W * H * 4) for _ in range(NL)]
            assert cd.decode_texture_segments_dev([f], dev, W * H * 4) is None
            assert b"".join(mem.to_host(p, U8, W * H * 4).tobytes() for p in dev) == want[0].tobytes(), kind
            fp, ln = files_arg([f]); dp = (C.c_void_p * NL)(*dev)
            assert cd.L.uvol_decode_texture_segments_dev(cd.h, fp, ln, 0, dp, W * H * 4) == uvol.UVOL_E_INVALID
            assert cd.L.uvol_decode_texture_segments_dev(cd.h, fp, ln, 1, None, W * H * 4) == uvol.UVOL_E_INVALID
            want, _ = cd.transcode_texture_segments_status([f], target="bc7")
            dev = [mem.alloc(4 * 16) for _ in range(NL)]; dp = (C.c_void_p * NL)(*dev)
            assert cd.L.uvol_transcode_texture_segments_bc7(cd.h, fp, ln, 1, dp, 4 * 16, 1) == uvol.UVOL_OK
            assert b"".join(mem.to_host(p, U8, 4 * 16).tobytes() for p in dev) == want[0].tobytes(), kind
        mem.free_all()
    finally:
        cd.close(); cu.close()


# ---------------------------------------------------------------------------------------------- texture encode forms
RAGGED = "all segments must have the same layer count and HxWx4 size"


def run_ragged_segments_refused(make):
    """Every form that takes nested host segments refuses ragged input (another layer count, another layer size) with one ValueError before
    the library sees a pointer, and nothing stays enqueued.  (Before the forms shared one intake only encode_texture_segments checked.)"""
    cd = make()
    try:
        a, b = tex_segments()
        for bad in ([a, b[:1]], [a, [b[0], b[1][:4]]]):
            for call in (cd.encode_texture_segments, cd.start_texture_segments, cd.encode_texture_segments_status, cd.encode_texture_segments_mips):
                with pytest.raises(ValueError) as e:
                    call(bad)
                assert str(e.value) == RAGGED, call.__name__
        assert cd.finish() == []
    finally:
        cd.close()


def run_texture_encode_forms(make, mem):
    """The blocking, _dev, _st, _mips(levels = 1) and enqueue forms give the same bytes on the same two segments, in an ETC1S context and
    in a UASTC context."""
    segs = tex_segments()
    for cfg in (dict(), dict(uastc=1)):
        cd = make(**cfg)
        try:
            want = cd.encode_texture_segments(segs)
            assert len(want) == 2 and all(want) and want[0] != want[1]
            assert [cd.encode_texture_segment(s) for s in segs] == want
            dev = [mem.to_dev(np.ascontiguousarray(a, dtype=U8)) for s in segs for a in s]
            assert cd.encode_texture_segments_dev(dev, NL, W, H) == want
            assert [cd.encode_texture_segment_dev(dev[k * NL:(k + 1) * NL], W, H) for k in range(2)] == want
            assert cd.encode_texture_segments_status(segs) == (want, [0, 0])
            assert cd.encode_texture_segments_mips(segs, levels=1) == (want, [0, 0])
            cd.start_texture_segments(segs); cd.start_texture_segments_dev(dev, NL, W, H)
            res = cd.finish()
            assert len(res) == 2 and res[0] == want and [bytes(v) for v in res[1]] == want, cfg
            mem.free_all()
        finally:
            cd.close()


# ---------------------------------------------------------------------------------------------- mesh enqueue
def run_mesh_enqueue(make):
    """start_mesh_batch + finish equal the blocking results for frames with and without face_mat; a face_material array of all NULLs
    through uvol_encode_mesh_batch_mat_async equals the plain form; a refused frame leaves its code in pending_status()."""
    import uvol
    cd = make(max_batch=2)
    try:
        ms = meshes5(); frames = [plain(m) for m in ms]; framesm = with_ids(ms)
        mixed = [frames[0], framesm[1], frames[2], framesm[3], frames[4]]
        want = [cd.encode_mesh_batch(fs) for fs in (frames, framesm, mixed)]
        cd.start_mesh_batch(frames); cd.start_mesh_batch(framesm); cd.start_mesh_batch(mixed); cd.start_mesh_batch(frames, slot=0); cd.start_mesh_batch(mixed, slot=1)
        sts = [list(cd.pending_status(k)) for k in range(5)]
        res = cd.finish()
        assert res[:3] == want and [[bytes(v) for v in r] for r in res[3:]] == [want[0], want[2]]
        assert sts == [[0] * 5] * 5
        # all NULLs through the _mat enqueue entry point
        n = len(frames); meshes = (uvol.Mesh * n)(); keep = []
        for i, f in enumerate(frames):
            meshes[i], k = cd._mesh_host(**f); keep.append(k)
        bufs = [np.zeros(cd.L.uvol_mesh_bound_mat(C.byref(meshes[i])), U8) for i in range(n)]
        outs = (C.c_void_p * n)(*[b.ctypes.data for b in bufs]); caps = (C.c_size_t * n)(*[b.size for b in bufs]); lens = (C.c_size_t * n)(); st = (C.c_int * n)(*([77] * n))
        for fm in ((C.c_void_p * n)(), None):
            assert cd.L.uvol_encode_mesh_batch_mat_async(cd.h, meshes, fm, n, 0, outs, caps, lens, st) == uvol.UVOL_OK
            assert cd.L.uvol_sync(cd.h) == uvol.UVOL_OK and list(st) == [0] * n
            assert [bufs[i][:lens[i]].tobytes() for i in range(n)] == want[0]
        assert cd.L.uvol_encode_mesh_batch_mat_async(cd.h, None, None, n, 0, outs, caps, lens, st) == uvol.UVOL_E_INVALID
        assert cd.L.uvol_encode_mesh_batch_mat_async(cd.h, meshes, (C.c_void_p * n)(), n, 0, None, caps, lens, st) == uvol.UVOL_E_INVALID
        # two materials that meet at a vertex: that frame is refused alone, its code stays in pending_status()
        bad = dict(frames[2], face_mat=(np.arange(nfaces(frames[2])) % 2).astype(U8))
        cd.start_mesh_batch([framesm[0], framesm[1], bad, framesm[3]])
        st = cd.pending_status()
        res = cd.finish()[0]
        assert list(st) == [0, 0, uvol.UVOL_E_UNSUPPORTED, 0] and res[2] is None
        assert [res[i] for i in (0, 1, 3)] == [want[1][i] for i in (0, 1, 3)]
        assert cd.encode_mesh_batch([framesm[0], bad], raise_on_error=False) == [want[1][0], None]
    finally:
        cd.close()


# ---------------------------------------------------------------------------------------------- the binding's RGBA-layer intake
WRONG_SIZE = "every layer must hold width * height * 4 bytes"


def run_binding_intake(make, mem):
    """downscale_rgba_batch_dev, mipchain_rgba_batch_dev and encode_etc2_rgb_batch accept arrays, bytes and bytearray, treat a list of
    ints as device pointers and raise ValueError with one text for a layer of the wrong size."""
    cd = make()
    try:
        lay = [np.ascontiguousarray(a, dtype=U8) for a in tex_segments()[0]]
        calls = dict(
            downscale=lambda x, **kw: [mem.to_host(p, U8, 4 * 4 * 4).tobytes() for p in cd.downscale_rgba_batch_dev(x, W, H, 2, **kw)],
            mipchain=lambda x, **kw: [[mem.to_host(p, U8, (W >> v) * (H >> v) * 4).tobytes() for v, p in enumerate(row, 1)] for row in cd.mipchain_rgba_batch_dev(x, W, H, **kw)],
            etc2=lambda x, **kw: [o.tobytes() for o in cd.encode_etc2_rgb_batch(x, W, H, **kw)])
        for name, call in calls.items():
            want = call(lay)
            assert len(want) == NL and want[0] != want[1], name
            assert call([a.tobytes() for a in lay]) == want, name
            assert call([bytearray(a.tobytes()) for a in lay]) == want, name
            assert call([lay[0], lay[1].tobytes()], on_device=False) == want, name
            dev = [int(mem.to_dev(a)) for a in lay]
            assert call(dev) == want and call(dev, on_device=True) == want, name
            assert call([]) == [], name
            for wrong in ([lay[0], lay[1][:7]], [lay[0].tobytes() + b"\0"], [bytearray(5)]):
                with pytest.raises(ValueError) as e:
                    call(wrong)
                assert str(e.value) == WRONG_SIZE, name
        mem.free_all()
    finally:
        cd.close()
