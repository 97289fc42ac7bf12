"""uvol.py — thin ctypes mirror of include/uvol_codec.h (libuvolcodec.so, HIP/gfx950).

Host-side counterpart of the two process boundaries of the reference driver
(scripts/Encoder.py:260-262 `draco_encoder`, :290-292 `basisu`).  There is no CPU fallback: if the
HIP library or a GPU is missing, `Codec()` raises.
"""
import ctypes as C
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(_HERE, "libuvolcodec.so")

UVOL_OK, UVOL_E_INVALID, UVOL_E_NODEVICE, UVOL_E_HIP, UVOL_E_NOSPACE, UVOL_E_ENCODE, UVOL_E_UNSUPPORTED = 0, -1, -2, -3, -4, -5, -6


class DecodedMesh(C.Structure):
    _fields_ = [("cap_faces", C.c_uint32), ("cap_values", C.c_size_t), ("pos", C.c_void_p), ("uv", C.c_void_p), ("nrm", C.c_void_p),
                ("idx_pos", C.c_void_p), ("idx_uv", C.c_void_p), ("idx_nrm", C.c_void_p),
                ("n_faces", C.c_uint32), ("n_pos", C.c_uint32), ("n_uv", C.c_uint32), ("n_nrm", C.c_uint32)]


class DecodedPoints(C.Structure):
    """uvol_decoded_points: the render-ready form of a decoded frame (one index per corner, one value record per point)."""
    _fields_ = [("cap_faces", C.c_uint32), ("cap_points", C.c_size_t), ("layout", C.c_uint32), ("pos", C.c_void_p), ("uv", C.c_void_p), ("nrm", C.c_void_p),
                ("index", C.c_void_p), ("n_faces", C.c_uint32), ("n_points", C.c_uint32), ("has_uv", C.c_uint32), ("has_nrm", C.c_uint32)]


UVOL_POINTS_PLANAR, UVOL_POINTS_INTERLEAVED = 0, 1


class PackedPoints(C.Structure):
    """uvol_packed_points: the render-ready form in 16-byte records of the file's own integers, with material ids."""
    _fields_ = [("cap_faces", C.c_uint32), ("cap_points", C.c_size_t), ("records", C.c_void_p), ("index", C.c_void_p),
                ("n_faces", C.c_uint32), ("n_points", C.c_uint32), ("has_uv", C.c_uint32), ("has_nrm", C.c_uint32), ("has_material", C.c_uint32),
                ("pos_bits", C.c_uint32), ("uv_bits", C.c_uint32), ("pos_min", C.c_float * 3), ("pos_scale", C.c_float), ("uv_min", C.c_float * 2), ("uv_scale", C.c_float)]


# one record of uvol_decode_mesh_batch_packed (16 bytes, little endian)
PACKED_RECORD = np.dtype([("pos", "<u2", 3), ("material", "<u2"), ("uv", "<u2", 2), ("nrm", "i1", 4)])


def packed_meta(m):
    """The output fields of one PackedPoints as a dict (counts, flags, the dequantisation transform as float32)."""
    return dict(n_faces=m.n_faces, n_points=m.n_points, has_uv=bool(m.has_uv), has_nrm=bool(m.has_nrm), has_material=bool(m.has_material),
                pos_bits=m.pos_bits, uv_bits=m.uv_bits, pos_min=np.array(m.pos_min[:], np.float32), pos_scale=np.float32(m.pos_scale),
                uv_min=np.array(m.uv_min[:], np.float32), uv_scale=np.float32(m.uv_scale))


class Params(C.Structure):
    """project-config.json numeric fields used on the hot path (scripts/Encoder.py:171-179)."""
    _fields_ = [("Q_POSITION_ATTR", C.c_int32), ("Q_TEXTURE_ATTR", C.c_int32), ("Q_NORMAL_ATTR", C.c_int32),
                ("Q_GENERIC_ATTR", C.c_int32), ("DRACO_COMPRESSION_LEVEL", C.c_int32), ("KTX2_BATCH_SIZE", C.c_int32),
                ("etc1s_quality", C.c_int32), ("y_flip", C.c_int32), ("max_batch", C.c_int32), ("cu_mod", C.c_int32), ("cu_residues", C.c_int32),
                ("traverse_vbits_l2", C.c_int32), ("stream_priority", C.c_int32), ("uastc", C.c_int32), ("material_seams", C.c_int32), ("reserved", C.c_int32 * 1)]


class Mesh(C.Structure):
    _fields_ = [("pos", C.c_void_p), ("n_pos", C.c_uint32), ("uv", C.c_void_p), ("n_uv", C.c_uint32),
                ("nrm", C.c_void_p), ("n_nrm", C.c_uint32), ("idx_pos", C.c_void_p), ("idx_uv", C.c_void_p),
                ("idx_nrm", C.c_void_p), ("n_faces", C.c_uint32)]


EXPORTS = ["uvol_params_default", "uvol_abi_version", "uvol_device_count", "uvol_ctx_create", "uvol_ctx_destroy",
           "uvol_last_error", "uvol_sync", "uvol_trim", "uvol_mesh_bound", "uvol_mesh_workspace", "uvol_encode_mesh", "uvol_encode_mesh_batch",
           "uvol_encode_mesh_batch_dev", "uvol_encode_mesh_batch_dev_out", "uvol_decode_mesh_batch_dev", "uvol_parse_obj_batch_dev", "uvol_unfilter_png_batch_dev", "uvol_encode_mesh_batch_async", "uvol_encode_mesh_batch_dev_async", "uvol_encode_texture_segments_async", "uvol_encode_texture_segments_dev_async", "uvol_texture_bound", "uvol_encode_texture_segment",
           "uvol_encode_texture_segment_dev", "uvol_encode_texture_segments", "uvol_encode_texture_segments_dev",
           "uvol_ktx2_info", "uvol_decode_texture_segments", "uvol_decode_texture_segments_dev", "uvol_transcode_texture_segments_etc1", "uvol_transcode_texture_segments_bc7", "uvol_transcode_texture_segments_etc2_rgba", "uvol_transcode_texture_segments_astc", "uvol_drc_info", "uvol_decode_mesh_batch", "uvol_profile_enable", "uvol_profile_reset", "uvol_profile_count",
           "uvol_profile_get", "uvol_encode_texture_segments_st", "uvol_transcode_texture_segments_st",
           "uvol_host_alloc", "uvol_host_free", "uvol_inflate_png_batch_dev", "uvol_png_status",
           "uvol_mesh_bound_mat", "uvol_encode_mesh_batch_mat", "uvol_encode_mesh_batch_mat_async", "uvol_decode_mesh_batch_mat", "uvol_parse_obj_batch_dev_mat",
           "uvol_decode_mesh_batch_points", "uvol_decode_mesh_batch_packed", "uvol_downscale_rgba_batch_dev",
           "uvol_etc2_rgb_bound", "uvol_encode_etc2_rgb_batch",
           "uvol_mip_level_count", "uvol_mipchain_rgba_batch_dev", "uvol_texture_bound_mips", "uvol_encode_texture_segments_mips", "uvol_ktx2_levels",
           "uvol_transcode_texture_segments_level",
           "uvol_jpeg_coeff_count", "uvol_idct_jpeg_batch_dev"]


class JpegLayout(C.Structure):
    """uvol_jpeg_layout: one layout for all images of a uvol_idct_jpeg_batch_dev call."""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("components", C.c_int), ("luma_h", C.c_int), ("luma_v", C.c_int)]


def load(path=None):
    path = path or os.environ.get("UVOL_LIB") or DEFAULT_LIB      # UVOL_LIB: diagnostic builds of the same HIP library (tools/)
    if not os.path.exists(path):
        raise RuntimeError(f"{path} not built: run __graft_entry__.build() (hipcc --offload-arch=gfx950); no CPU fallback exists")
    L = C.CDLL(path)
    L.uvol_params_default.argtypes = [C.POINTER(Params)]
    L.uvol_ctx_create.argtypes = [C.c_int, C.POINTER(Params), C.POINTER(C.c_void_p)]
    L.uvol_ctx_destroy.argtypes = [C.c_void_p]
    L.uvol_last_error.argtypes = [C.c_void_p]; L.uvol_last_error.restype = C.c_char_p
    L.uvol_sync.argtypes = [C.c_void_p]
    L.uvol_trim.argtypes = [C.c_void_p]
    L.uvol_mesh_bound.argtypes = [C.POINTER(Mesh)]; L.uvol_mesh_bound.restype = C.c_size_t
    L.uvol_mesh_workspace.argtypes = [C.c_void_p, C.POINTER(Mesh)]; L.uvol_mesh_workspace.restype = C.c_size_t
    L.uvol_encode_mesh.argtypes = [C.c_void_p, C.POINTER(Mesh), C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    for nm in ("uvol_encode_mesh_batch", "uvol_encode_mesh_batch_dev", "uvol_encode_mesh_batch_async", "uvol_encode_mesh_batch_dev_async"):
        getattr(L, nm).argtypes = [C.c_void_p, C.POINTER(Mesh), C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                   C.POINTER(C.c_size_t), C.POINTER(C.c_int)]
    L.uvol_mesh_bound_mat.argtypes = [C.POINTER(Mesh)]; L.uvol_mesh_bound_mat.restype = C.c_size_t
    for nm in ("uvol_encode_mesh_batch_mat", "uvol_encode_mesh_batch_mat_async"):
        getattr(L, nm).argtypes = [C.c_void_p, C.POINTER(Mesh), C.POINTER(C.c_void_p), C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                   C.POINTER(C.c_size_t), C.POINTER(C.c_int)]
    L.uvol_decode_mesh_batch_mat.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int, C.c_int, C.POINTER(DecodedMesh),
                                             C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    if hasattr(L, "uvol_decode_mesh_batch_points"):      # (a build that predates the entry point still loads: tools/points_timing.py times one beside this build)
        L.uvol_decode_mesh_batch_points.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int, C.c_int, C.POINTER(DecodedPoints), C.POINTER(C.c_int)]
    if hasattr(L, "uvol_decode_mesh_batch_packed"):      # (the same: tools/points_timing.py loads the parent build beside this one)
        L.uvol_decode_mesh_batch_packed.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int, C.c_int, C.POINTER(PackedPoints), C.POINTER(C.c_int)]
    L.uvol_parse_obj_batch_dev_mat.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int, C.c_int, C.POINTER(Mesh), C.POINTER(C.c_void_p), C.POINTER(C.c_int)]
    L.uvol_texture_bound.argtypes = [C.c_uint32, C.c_uint32, C.c_int]; L.uvol_texture_bound.restype = C.c_size_t
    for nm in ("uvol_encode_texture_segment", "uvol_encode_texture_segment_dev"):
        getattr(L, nm).argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_uint32, C.c_uint32, C.c_void_p,
                                   C.c_size_t, C.POINTER(C.c_size_t)]
    for nm in ("uvol_encode_texture_segments", "uvol_encode_texture_segments_dev", "uvol_encode_texture_segments_async", "uvol_encode_texture_segments_dev_async"):
        getattr(L, nm).argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p),
                                   C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.uvol_ktx2_info.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    for nm in ("uvol_decode_texture_segments", "uvol_decode_texture_segments_dev"):
        getattr(L, nm).argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int, C.POINTER(C.c_void_p), C.c_size_t]
    L.uvol_transcode_texture_segments_etc1.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int, C.POINTER(C.c_void_p), C.c_size_t, C.c_int]
    L.uvol_transcode_texture_segments_bc7.argtypes = L.uvol_transcode_texture_segments_etc1.argtypes
    L.uvol_transcode_texture_segments_astc.argtypes = L.uvol_transcode_texture_segments_etc1.argtypes
    L.uvol_transcode_texture_segments_etc2_rgba.argtypes = L.uvol_transcode_texture_segments_etc1.argtypes
    L.uvol_encode_texture_segments_st.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_void_p),
                                                  C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_int)]
    L.uvol_transcode_texture_segments_st.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int, C.POINTER(C.c_void_p), C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_int)]
    L.uvol_host_alloc.argtypes = [C.c_size_t]; L.uvol_host_alloc.restype = C.c_void_p
    L.uvol_host_free.argtypes = [C.c_void_p]
    L.uvol_drc_info.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.uvol_decode_mesh_batch.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int, C.POINTER(DecodedMesh), C.POINTER(C.c_int)]
    L.uvol_decode_mesh_batch_dev.argtypes = L.uvol_decode_mesh_batch.argtypes
    L.uvol_unfilter_png_batch_dev.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    L.uvol_inflate_png_batch_dev.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    L.uvol_png_status.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_int]
    L.uvol_downscale_rgba_batch_dev.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    if hasattr(L, "uvol_encode_etc2_rgb_batch"):      # (a build that predates the entry point still loads: tools/etc2_direct_timing.py may time one beside this build)
        L.uvol_etc2_rgb_bound.argtypes = [C.c_uint32, C.c_uint32]; L.uvol_etc2_rgb_bound.restype = C.c_size_t
        L.uvol_encode_etc2_rgb_batch.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_void_p), C.c_size_t, C.c_int]
    if hasattr(L, "uvol_mipchain_rgba_batch_dev"):      # (a build that predates the mip levels still loads: tools/mipchain_timing.py may time one beside this build)
        L.uvol_mip_level_count.argtypes = [C.c_uint32, C.c_uint32]
        L.uvol_mipchain_rgba_batch_dev.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.uvol_texture_bound_mips.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.c_int]; L.uvol_texture_bound_mips.restype = C.c_size_t
        L.uvol_encode_texture_segments_mips.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.POINTER(C.c_void_p),
                                                        C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_int)]
        L.uvol_ktx2_levels.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_uint32)]
        L.uvol_transcode_texture_segments_level.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int, C.c_int, C.POINTER(C.c_void_p), C.c_size_t, C.c_int, C.c_int, C.POINTER(C.c_int)]
    if hasattr(L, "uvol_idct_jpeg_batch_dev"):      # (a build that predates the JPEG ingest still loads beside this one)
        L.uvol_jpeg_coeff_count.argtypes = [C.POINTER(JpegLayout)]; L.uvol_jpeg_coeff_count.restype = C.c_size_t
        L.uvol_idct_jpeg_batch_dev.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int, C.POINTER(JpegLayout), C.c_int, C.POINTER(C.c_void_p)]
    L.uvol_parse_obj_batch_dev.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int, C.c_int, C.POINTER(Mesh), C.POINTER(C.c_int)]
    L.uvol_encode_mesh_batch_dev_out.argtypes = [C.c_void_p, C.POINTER(Mesh), C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_int)]
    L.uvol_profile_enable.argtypes = [C.c_void_p, C.c_int]
    L.uvol_profile_reset.argtypes = [C.c_void_p]
    L.uvol_profile_count.argtypes = [C.c_void_p]
    L.uvol_profile_get.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_uint64),
                                   C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    return L


class UvolError(RuntimeError):
    pass


class PinnedArena:
    """Page-locked host memory from uvol_host_alloc, handed out as numpy arrays (the arrays must not outlive the arena).  Inputs that ALL lie
    in such memory are uploaded without the library's staging copy."""

    def __init__(self, nbytes, lib_path=None):
        self.L = load(lib_path); self.n = int(nbytes); self.off = 0
        self.p = self.L.uvol_host_alloc(self.n)
        if not self.p:
            raise UvolError(f"uvol_host_alloc({self.n}) failed")
        self.buf = (C.c_uint8 * self.n).from_address(self.p)

    def put(self, a):
        a = np.ascontiguousarray(a); nb = a.nbytes; o = (self.off + 255) & ~255
        if o + nb > self.n:
            raise UvolError("pinned arena full")
        v = np.frombuffer(self.buf, dtype=a.dtype, count=a.size, offset=o).reshape(a.shape)
        v[...] = a; self.off = o + nb
        return v

    def take(self, shape, dtype):
        """An uninitialised array of this shape in the arena (256-byte aligned)."""
        dt = np.dtype(dtype); cnt = int(np.prod(shape)); nb = cnt * dt.itemsize; o = (self.off + 255) & ~255
        if o + nb > self.n:
            raise UvolError("pinned arena full")
        self.off = o + nb
        return np.frombuffer(self.buf, dtype=dt, count=cnt, offset=o).reshape(shape)

    def close(self):
        if getattr(self, "p", None):
            self.buf = None; self.L.uvol_host_free(self.p); self.p = None

    __del__ = close


def _f32(a, cols):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float32).reshape(-1, cols)


def _u32(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.uint32).reshape(-1)


def _files(files):
    """The file-list arguments of the ABI -> (the files as bytes, the char* array, the length array, their count)."""
    files = [bytes(f) for f in files]; n = len(files)
    return files, (C.c_char_p * n)(*files), (C.c_size_t * n)(*[len(f) for f in files]), n


def _layers(items, width, height, on_device):
    """The RGBA-layer intake of the batch calls on layers of one size: device pointers (ints), or host images (HxWx4 uint8 arrays / bytes of
    width * height * 4), which the library uploads.  on_device=None: device pointers when every entry is an int.
    -> (the void* array, the host arrays it points into, on_device)"""
    items = list(items); n = len(items)
    if on_device is None:
        on_device = n > 0 and all(isinstance(x, int) for x in items)
    if on_device:
        return (C.c_void_p * n)(*[int(p) if p else None for p in items]), [], True
    keep = []
    for a in items:
        if a is None:
            keep.append(None); continue
        a = np.ascontiguousarray(np.frombuffer(a, np.uint8) if isinstance(a, (bytes, bytearray)) else a, dtype=np.uint8)
        if a.size != width * height * 4:
            raise ValueError("every layer must hold width * height * 4 bytes")
        keep.append(a)
    return (C.c_void_p * n)(*[a.ctypes.data if a is not None else None for a in keep]), keep, False


def _segments(segments):
    """Host texture segments (lists of HxWx4 uint8 arrays, one size, one layer count) -> (the arrays in one list, their void* array, width,
    height, layers per segment, segments)."""
    arrs = [[np.ascontiguousarray(a, dtype=np.uint8) for a in seg] for seg in segments]
    h, w = arrs[0][0].shape[:2]; nl = len(arrs[0])
    flat = [a for seg in arrs for a in seg]
    if any(len(seg) != nl for seg in arrs) or any(a.shape != (h, w, 4) for a in flat):
        raise ValueError("all segments must have the same layer count and HxWx4 size")
    return flat, (C.c_void_p * len(flat))(*[a.ctypes.data for a in flat]), w, h, nl, len(arrs)


class Codec:
    """One codec context = one GPU + one HIP stream.  Field names follow project-config.json."""

    def __init__(self, device=0, lib_path=None, **config):
        self.L = load(lib_path)
        p = Params()
        self.L.uvol_params_default(C.byref(p))
        for k, v in config.items():
            if not hasattr(p, k):
                raise KeyError(k)
            setattr(p, k, int(v))
        self.params = p
        h = C.c_void_p()
        rc = self.L.uvol_ctx_create(device, C.byref(p), C.byref(h))
        if rc != UVOL_OK:
            raise UvolError(f"uvol_ctx_create(device={device}) failed rc={rc} (no CPU fallback; a gfx950 GPU is required)")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.uvol_ctx_destroy(self.h)
            self.h = None

    __del__ = close

    def error(self):
        return self.L.uvol_last_error(self.h).decode()

    # ---- geometry ----
    @staticmethod
    def _mesh_host(pos, idx_pos, uv=None, idx_uv=None, nrm=None, idx_nrm=None):
        pos = _f32(pos, 3); uv = _f32(uv, 2); nrm = _f32(nrm, 3)
        idx_pos = _u32(idx_pos); idx_uv = _u32(idx_uv); idx_nrm = _u32(idx_nrm)
        m = Mesh()
        m.pos = pos.ctypes.data; m.n_pos = len(pos)
        m.idx_pos = idx_pos.ctypes.data; m.n_faces = len(idx_pos) // 3
        if uv is not None and idx_uv is not None:
            m.uv = uv.ctypes.data; m.n_uv = len(uv); m.idx_uv = idx_uv.ctypes.data
        if nrm is not None and idx_nrm is not None:
            m.nrm = nrm.ctypes.data; m.n_nrm = len(nrm); m.idx_nrm = idx_nrm.ctypes.data
        return m, (pos, uv, nrm, idx_pos, idx_uv, idx_nrm)

    @staticmethod
    def _mesh_host_mat(face_mat=None, **f):
        """_mesh_host of a frame dict that may carry "face_mat" (one uint8 material id per face) -> (Mesh, its arrays, the id array or None)."""
        m, keep = Codec._mesh_host(**f)
        face_mat = None if face_mat is None else np.ascontiguousarray(face_mat, dtype=np.uint8).reshape(-1)
        if face_mat is not None and len(face_mat) != m.n_faces:
            raise ValueError("face_mat: one material id per face")
        return m, keep, face_mat

    @staticmethod
    def _mat_ptrs(mats):
        """The parallel face_material array of the _mat entry points (None when no frame has ids: the plain entry points are called)."""
        if all(a is None for a in mats):
            return None
        return (C.c_void_p * len(mats))(*[(None if a is None else a.ctypes.data) for a in mats])

    def mesh_workspace(self, pos, idx_pos, uv=None, idx_uv=None, nrm=None, idx_nrm=None) -> int:
        """Device bytes one frame of these dimensions holds while in flight."""
        m, keep = self._mesh_host(pos, idx_pos, uv, idx_uv, nrm, idx_nrm)
        return int(self.L.uvol_mesh_workspace(self.h, C.byref(m)))

    def encode_mesh(self, pos, idx_pos, uv=None, idx_uv=None, nrm=None, idx_nrm=None, face_mat=None) -> bytes:
        return self.encode_mesh_batch([dict(pos=pos, idx_pos=idx_pos, uv=uv, idx_uv=idx_uv, nrm=nrm, idx_nrm=idx_nrm, face_mat=face_mat)])[0]

    def encode_mesh_batch(self, frames, raise_on_error=True, views=False):
        """frames: list of dicts(pos, idx_pos[, uv, idx_uv, nrm, idx_nrm, face_mat]) of host arrays -> list of .drc bytes (views=True: numpy
        views of this codec's output buffers, valid until the next call).  face_mat: one uint8 material id per face (the OBJ `usemtl`
        attribute, uvol_encode_mesh_batch_mat); a frame in which two materials meet at a vertex fails alone with UVOL_E_UNSUPPORTED."""
        n = len(frames)
        meshes = (Mesh * n)(); keep = []; fms = []
        for i, f in enumerate(frames):
            m, k, fm = self._mesh_host_mat(**f); meshes[i] = m; keep.append(k); fms.append(fm)
        mats = self._mat_ptrs(fms)
        if mats is None:
            return self._run_batch(self.L.uvol_encode_mesh_batch, meshes, n, raise_on_error, views)
        fn = lambda h, ms, nn, outs, caps, lens, st: self.L.uvol_encode_mesh_batch_mat(h, ms, mats, nn, 0, outs, caps, lens, st)
        return self._run_batch(fn, meshes, n, raise_on_error, views, bound=self.L.uvol_mesh_bound_mat)

    def encode_mesh_batch_dev_mat(self, meshes, mats, raise_on_error=True, views=False):
        """As encode_mesh_batch_dev, with material ids resident in HBM: mats = list of device pointers (ints, None = no ids for that frame)."""
        mp = (C.c_void_p * len(meshes))(*[(None if p is None else int(p)) for p in mats])
        fn = lambda h, ms, nn, outs, caps, lens, st: self.L.uvol_encode_mesh_batch_mat(h, ms, mp, nn, 1, outs, caps, lens, st)
        return self._run_batch(fn, meshes, len(meshes), raise_on_error, views, bound=self.L.uvol_mesh_bound_mat)

    def encode_mesh_batch_dev(self, meshes, raise_on_error=True, views=False):
        """meshes: ctypes array of Mesh holding DEVICE pointers (inputs resident in HBM).  views=True: numpy views of this
        codec's output buffers instead of `bytes` copies (valid until the next call; no 250 KB copy per frame in Python)."""
        return self._run_batch(self.L.uvol_encode_mesh_batch_dev, meshes, len(meshes), raise_on_error, views)

    def encode_mesh_batch_dev_out(self, meshes, dev_out, dev_cap, producer_stream=None):
        """GPU-resident form: `meshes` hold device pointers produced on `producer_stream` (a hipStream_t as an int, None = complete), the
        .drc bitstreams stay in HBM, packed into the caller's device buffer.  -> (offsets, lengths, statuses) as lists."""
        n = len(meshes)
        offs = (C.c_size_t * n)(); lens = (C.c_size_t * n)(); st = (C.c_int * n)()
        rc = self.L.uvol_encode_mesh_batch_dev_out(self.h, meshes, n, C.c_void_p(producer_stream or 0), C.c_void_p(int(dev_out)), int(dev_cap), offs, lens, st)
        if rc != UVOL_OK:
            raise UvolError(f"encode_mesh_batch_dev_out rc={rc}: {self.error()}")
        return list(offs), list(lens), list(st)

    def decode_mesh_batch_dev(self, files, metas):
        """files: list of .drc bytes; metas: ctypes array of DecodedMesh whose buffers are DEVICE pointers (capacities filled in by the
        caller, see uvol_drc_info): the decoded arrays stay in HBM, the counts come back in `metas`.  -> list of statuses."""
        files, fp, ln, n = _files(files); st = (C.c_int * n)()
        rc = self.L.uvol_decode_mesh_batch_dev(self.h, fp, ln, n, metas, st)
        if rc != UVOL_OK:
            raise UvolError(f"decode_mesh_batch_dev rc={rc}: {self.error()}")
        return list(st)

    def parse_obj_batch_dev(self, texts, slot=0):
        """texts: list of OBJ files as bytes -> (ctypes array of Mesh with DEVICE pointers into the context's slot, list of statuses)."""
        texts, tp, ln, n = _files(texts); meshes = (Mesh * n)(); st = (C.c_int * n)()
        rc = self.L.uvol_parse_obj_batch_dev(self.h, tp, ln, n, slot, meshes, st)
        if rc != UVOL_OK:
            raise UvolError(f"parse_obj_batch_dev rc={rc}: {self.error()}")
        return meshes, list(st)

    def unfilter_png_batch_dev(self, inflated, width, height, channels, slot=0, sync=True):
        """inflated: list of bytes (the inflated IDAT stream of 8-bit RGB / RGBA PNGs of one size) -> list of DEVICE pointers to RGBA8 layers.
        sync=False: return once the kernel is queued (this context's texture entry points order themselves behind it)."""
        raws, rp, _, n = _files(inflated); out = (C.c_void_p * n)()
        rc = self.L.uvol_unfilter_png_batch_dev(self.h, rp, n, width, height, channels, slot, out)
        if rc != UVOL_OK:
            raise UvolError(f"unfilter_png_batch_dev rc={rc}: {self.error()}")
        if sync and self.L.uvol_sync(self.h) != UVOL_OK:
            raise UvolError(f"uvol_sync: {self.error()}")
        return [int(p) for p in out]

    def inflate_png_batch_dev(self, zstreams, width, height, channels, slot=0, sync=True):
        """zstreams: list of bytes (the zlib stream = concatenated IDAT data of 8-bit RGB / RGBA PNGs of one size) -> (list of DEVICE pointers
        to RGBA8 layers, list of per-image statuses); inflate and un-filter both run on the device."""
        zs, zp, ln, n = _files(zstreams); out = (C.c_void_p * n)(); st = (C.c_int * n)()
        rc = self.L.uvol_inflate_png_batch_dev(self.h, zp, ln, n, width, height, channels, slot, out)
        if rc != UVOL_OK:
            raise UvolError(f"inflate_png_batch_dev rc={rc}: {self.error()}")
        rc = self.L.uvol_png_status(self.h, slot, st, n)
        if rc != UVOL_OK:
            raise UvolError(f"png_status rc={rc}: {self.error()}")
        if sync and self.L.uvol_sync(self.h) != UVOL_OK:
            raise UvolError(f"uvol_sync: {self.error()}")
        return [int(p) for p in out], list(st)

    def jpeg_coeff_count(self, width, height, components, luma_h=1, luma_v=1):
        """uvol_jpeg_coeff_count: int16 values per image of that layout (0: a layout outside the rule)."""
        lay = JpegLayout(width, height, components, luma_h, luma_v)
        return int(self.L.uvol_jpeg_coeff_count(C.byref(lay)))

    def idct_jpeg_batch_dev(self, coeffs, qtables, width, height, components, luma_h=1, luma_v=1, slot=0, sync=True):
        """uvol_idct_jpeg_batch_dev: coeffs[i] = the quantised coefficients of image i (int16, uvol_jpeg_coeff_count values, the layout of
        include/uvol_codec.h), qtables[i] = its components x 64 quantisation values (uint16) -> list of DEVICE pointers to the RGBA8 layers in the
        ingest slot.  Arrays are passed where they lie (arrays of a PinnedArena are read without the staging copy); None stands for NULL.
        sync=False: return once the kernels are queued (this context's texture entry points order themselves behind them)."""
        n = len(coeffs if coeffs is not None else qtables); keep = []

        def ptrs(items, dt):
            out = []
            for a in items:
                if a is None:
                    out.append(None); continue
                if not (isinstance(a, np.ndarray) and a.dtype == dt and a.flags.c_contiguous):
                    a = np.ascontiguousarray(a, dtype=dt)
                keep.append(a); out.append(a.ctypes.data)
            return (C.c_void_p * len(out))(*out)
        cp = ptrs(coeffs, np.int16) if coeffs is not None else None
        qp = ptrs(qtables, np.uint16) if qtables is not None else None
        lay = JpegLayout(width, height, components, luma_h, luma_v); out = (C.c_void_p * max(n, 1))()
        rc = self.L.uvol_idct_jpeg_batch_dev(self.h, cp, qp, n, C.byref(lay), slot, out)
        if rc != UVOL_OK:
            raise UvolError(f"idct_jpeg_batch_dev rc={rc}: {self.error()}")
        if sync and self.L.uvol_sync(self.h) != UVOL_OK:
            raise UvolError(f"uvol_sync: {self.error()}")
        return [int(p) for p in out[:n]]

    def downscale_rgba_batch_dev(self, layers_or_ptrs, width, height, factor, slot=0, on_device=None):
        """uvol_downscale_rgba_batch_dev: layers of one size, downscaled by factor 2 / 4 / 8 on the device -> list of DEVICE pointers to the
        ceil(width / factor) x ceil(height / factor) RGBA8 layers in the context's downscale slot (valid until that slot is written again;
        what encode_texture_segment[s]_dev takes).  layers_or_ptrs: device pointers (ints), or host images (HxWx4 uint8 arrays / bytes of
        width * height * 4), which are uploaded.  on_device=None: device pointers when every entry is an int."""
        ptrs, keep, on_device = _layers(layers_or_ptrs, width, height, on_device); n = len(ptrs)
        out = (C.c_void_p * n)()
        rc = self.L.uvol_downscale_rgba_batch_dev(self.h, ptrs, n, width, height, 1 if on_device else 0, factor, slot, out)
        if rc != UVOL_OK:
            raise UvolError(f"downscale_rgba_batch_dev rc={rc}: {self.error()}")
        return [int(p) for p in out]

    def mip_level_count(self, width, height):
        """uvol_mip_level_count: floor(log2(max(width, height))) + 1, level 0 included."""
        return int(self.L.uvol_mip_level_count(width, height))

    def mipchain_rgba_batch_dev(self, layers_or_ptrs, width, height, levels=0, slot=0, on_device=None):
        """uvol_mipchain_rgba_batch_dev: layers of one size -> their mip levels 1 .. levels - 1 (levels=0: the full chain), made on the device in
        one pass over level 0.  Returns one list per layer of DEVICE pointers, entry v - 1 = level v (max(1, width >> v) x max(1, height >> v)
        RGBA8) in the context's chain slot, valid until that slot is written again.  layers_or_ptrs / on_device as downscale_rgba_batch_dev."""
        ptrs, keep, on_device = _layers(layers_or_ptrs, width, height, on_device); n = len(ptrs)
        full = max(self.mip_level_count(width, height), 1)
        nl = levels if 1 <= levels <= full else full          # (the array is sized for the longest chain; the library judges `levels`)
        out = (C.c_void_p * max(n * (full - 1), 1))()
        rc = self.L.uvol_mipchain_rgba_batch_dev(self.h, ptrs, n, width, height, 1 if on_device else 0, levels, slot, out)
        if rc != UVOL_OK:
            raise UvolError(f"mipchain_rgba_batch_dev rc={rc}: {self.error()}")
        return [[int(out[i * (nl - 1) + v]) for v in range(nl - 1)] for i in range(n)]

    def encode_etc2_rgb_batch(self, layers_or_ptrs, width, height, on_device=None, out_dev_ptrs=None, layer_cap=None):
        """uvol_encode_etc2_rgb_batch: RGBA8 layers of one size -> full ETC1 blocks (valid ETC2 RGB8) searched from the source texels, one launch
        for the batch.  layers_or_ptrs: device pointers (ints), or host images (HxWx4 uint8 arrays / bytes of width * height * 4), which are
        uploaded; on_device=None: device pointers when every entry is an int.  Returns a list of [by, bx, 8] uint8 arrays - or, with
        out_dev_ptrs (one 8-byte aligned device buffer of uvol_etc2_rgb_bound bytes per layer), writes there and returns None.  layer_cap:
        the size of each output buffer when it is not the bound."""
        ptrs, keep, on_device = _layers(layers_or_ptrs, width, height, on_device); n = len(ptrs)
        bx, by = (width + 3) // 4, (height + 3) // 4
        cap = bx * by * 8 if layer_cap is None else layer_cap
        if out_dev_ptrs is not None:
            outs = None; op = (C.c_void_p * n)(*[int(p) if p else None for p in out_dev_ptrs])
        else:
            outs = [np.empty((by, bx, 8), dtype=np.uint8) for _ in range(n)]; op = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
        rc = self.L.uvol_encode_etc2_rgb_batch(self.h, ptrs, n, width, height, 1 if on_device else 0, op, cap, 0 if outs is not None else 1)
        if rc != UVOL_OK:
            raise UvolError(f"encode_etc2_rgb_batch rc={rc}: {self.error()}")
        return outs

    def drc_info(self, data):
        nf, mv = C.c_uint32(), C.c_uint32()
        if self.L.uvol_drc_info(bytes(data), len(data), C.byref(nf), C.byref(mv)) != UVOL_OK:
            raise UvolError("not a .drc this decoder handles")
        return nf.value, mv.value

    # ---- enqueue form (uvol_*_async + uvol_sync): start_* record a call, finish() completes all of them in order ----
    def start_mesh_batch(self, frames, slot=None):
        """Enqueues uvol_encode_mesh_batch_async for host frames; the result arrives with finish().  slot=None: fresh output buffers, finish()
        returns `bytes`; slot=k: the output buffers of slot k are re-used by every call with that slot and finish() returns numpy views into
        them (two slots let consecutive enqueued calls overlap without a buffer set - and its page faults - per call)."""
        n = len(frames)
        meshes = (Mesh * n)(); keep = []; fms = []
        for i, f in enumerate(frames):
            m, k, fm = self._mesh_host_mat(**f); meshes[i] = m; keep.append(k); fms.append(fm)
        mats = self._mat_ptrs(fms); lens = (C.c_size_t * n)(); st = (C.c_int * n)()
        bufs, outs, caps = self._slot_bufs(None if slot is None else ("mesh", "host", slot), n, self.L.uvol_mesh_bound if mats is None else self.L.uvol_mesh_bound_mat, meshes)
        if mats is None:
            rc = self.L.uvol_encode_mesh_batch_async(self.h, meshes, n, outs, caps, lens, st)
        else:
            rc = self.L.uvol_encode_mesh_batch_mat_async(self.h, meshes, mats, n, 0, outs, caps, lens, st)
        if rc != UVOL_OK:
            raise UvolError(f"encode_mesh_batch_async rc={rc}: {self.error()}")
        self._pending = getattr(self, "_pending", []) + [("mesh" if slot is None else "mesh_views", n, bufs, lens, st, (keep, fms, mats), meshes)]

    def start_mesh_batch_dev(self, meshes, slot=0):
        """Enqueues uvol_encode_mesh_batch_dev_async for a ctypes array of Mesh holding DEVICE pointers.  The output buffers of `slot`
        are re-used by every call with that slot (two slots let consecutive enqueued calls overlap without a buffer set per call);
        finish() returns numpy views into them."""
        n = len(meshes); lens = (C.c_size_t * n)(); st = (C.c_int * n)()
        bufs, outs, caps = self._slot_bufs(("mesh", "dev", slot), n, self.L.uvol_mesh_bound, meshes)
        rc = self.L.uvol_encode_mesh_batch_dev_async(self.h, meshes, n, outs, caps, lens, st)
        if rc != UVOL_OK:
            raise UvolError(f"encode_mesh_batch_dev_async rc={rc}: {self.error()}")
        self._pending = getattr(self, "_pending", []) + [("mesh_views", n, bufs, lens, st, (caps, outs), meshes)]

    def _slot_bufs(self, key, n, bound=None, meshes=None, cap=None):
        """The output arguments of a batch call: n buffers of the set `key`, which is kept between calls and re-used by every call with that key
        (no fresh pages to fault in per batch; None: fresh buffers), each grown to bound(meshes[i]) - meshes - or to `cap` - textures.
        -> (the buffers, the void* array, the capacity array)"""
        bufs = [] if key is None else self.__dict__.setdefault("_out_bufs", {}).setdefault(key, [])
        while len(bufs) < n:
            bufs.append(np.empty(0, dtype=np.uint8))
        caps = (C.c_size_t * n)(); outs = (C.c_void_p * n)()
        for i, c in enumerate([cap] * n if bound is None else [bound(C.byref(meshes[i])) for i in range(n)]):
            if bufs[i].size < c:
                bufs[i] = np.empty(c, dtype=np.uint8)
            caps[i] = c; outs[i] = bufs[i].ctypes.data
        return bufs, outs, caps

    def start_texture_segments(self, segments, slot=None):
        """Enqueues uvol_encode_texture_segments_async for host segments (slot: as in start_mesh_batch)."""
        flat, ptrs, w, h, nl, nseg = _segments(segments); lens = (C.c_size_t * nseg)()
        bufs, outs, caps = self._slot_bufs(None if slot is None else ("tex", slot), nseg, cap=self.L.uvol_texture_bound(w, h, nl))
        rc = self.L.uvol_encode_texture_segments_async(self.h, ptrs, nseg, nl, w, h, outs, caps, lens)
        if rc != UVOL_OK:
            raise UvolError(f"encode_texture_segments_async rc={rc}: {self.error()}")
        self._pending = getattr(self, "_pending", []) + [("tex" if slot is None else "tex_views", nseg, bufs, lens, None, flat, ptrs)]

    def start_texture_segments_dev(self, dev_ptrs, n_layers, width, height, slot=0):
        """Enqueues uvol_encode_texture_segments_dev_async for a flat list of n_segments * n_layers DEVICE pointers; output buffers of `slot`
        are re-used, finish() returns numpy views."""
        ptrs = (C.c_void_p * len(dev_ptrs))(*[int(p) for p in dev_ptrs]); nseg = len(dev_ptrs) // n_layers; lens = (C.c_size_t * nseg)()
        bufs, outs, caps = self._slot_bufs(("tex", "dev", slot), nseg, cap=self.L.uvol_texture_bound(width, height, n_layers))
        rc = self.L.uvol_encode_texture_segments_dev_async(self.h, ptrs, nseg, n_layers, width, height, outs, caps, lens)
        if rc != UVOL_OK:
            raise UvolError(f"encode_texture_segments_dev_async rc={rc}: {self.error()}")
        self._pending = getattr(self, "_pending", []) + [("tex_views", nseg, bufs, lens, None, None, ptrs)]

    def pending_status(self, k=-1):
        """The status array (ctypes ints, one per frame) of the k-th enqueued mesh call that finish() has not completed yet: finish()
        reports a failed frame as None only, its code stays here."""
        return self._pending[k][4]

    def trim(self):
        """uvol_trim: completes the context's work and gives its geometry workspaces back to the device (streams stay)."""
        rc = self.L.uvol_trim(self.h)
        if rc != UVOL_OK:
            raise UvolError(f"uvol_trim rc={rc}: {self.error()}")

    def finish(self):
        """uvol_sync: completes every enqueued call; returns their results in call order (meshes: None for a failed frame)."""
        rc = self.L.uvol_sync(self.h)
        pend, self._pending = getattr(self, "_pending", []), []
        res = []
        for kind, n, bufs, lens, st, _, _ in pend:
            if kind == "mesh_views":
                res.append([(bufs[i][:lens[i]] if st[i] == UVOL_OK else None) for i in range(n)])
            elif kind == "tex_views":
                res.append([(bufs[i][:lens[i]] if lens[i] else None) for i in range(n)])
            else:
                res.append([(bufs[i][:lens[i]].tobytes() if ((st is None or st[i] == UVOL_OK) and lens[i]) else None) for i in range(n)])
        if rc != UVOL_OK:
            # a call that failed as a whole leaves its lengths at zero (entries None); the calls that succeeded are not lost with it
            e = UvolError(f"uvol_sync rc={rc}: {self.error()}"); e.partial_results = res
            raise e
        return res

    def _run_batch(self, fn, meshes, n, raise_on_error, views=False, bound=None):
        lens = (C.c_size_t * n)(); st = (C.c_int * n)()
        bufs, outs, caps = self._slot_bufs(("mesh", "blocking"), n, bound or self.L.uvol_mesh_bound, meshes)
        rc = fn(self.h, meshes, n, outs, caps, lens, st)
        if rc != UVOL_OK:
            raise UvolError(f"encode_mesh_batch rc={rc}: {self.error()}")
        res = []
        for i in range(n):
            if st[i] != UVOL_OK:
                if raise_on_error:
                    raise UvolError(f"frame {i} failed status={st[i]}: {self.error()}")
                res.append(None)
            else:
                res.append(bufs[i][:lens[i]] if views else bufs[i][:lens[i]].tobytes())
        return res

    # ---- texture ----
    def encode_texture_segment(self, layers) -> bytes:
        """layers: list of HxWx4 uint8 arrays (top row first) -> one .ktx2 (ETC1S/BasisLZ, len(layers) array layers)."""
        arrs = [np.ascontiguousarray(a, dtype=np.uint8) for a in layers]
        h, w = arrs[0].shape[:2]
        for a in arrs:
            if a.shape != (h, w, 4):
                raise ValueError("all layers must be HxWx4 uint8 of one size")
        n = len(arrs)
        ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in arrs])
        return self._run_tex(self.L.uvol_encode_texture_segment, ptrs, n, w, h)

    def encode_texture_segment_dev(self, dev_ptrs, width, height) -> bytes:
        n = len(dev_ptrs)
        ptrs = (C.c_void_p * n)(*[int(p) for p in dev_ptrs])
        return self._run_tex(self.L.uvol_encode_texture_segment_dev, ptrs, n, width, height)

    def encode_texture_segments(self, segments, views=False):
        """segments: list of lists of HxWx4 uint8 arrays (same size, same layer count) -> list of .ktx2 bytes (one batched call;
        views=True: numpy views of this codec's output buffers, valid until the next call)."""
        flat, ptrs, w, h, nl, nseg = _segments(segments)
        return self._run_tex_batch(self.L.uvol_encode_texture_segments, ptrs, nseg, nl, w, h, views)

    def encode_texture_segments_dev(self, dev_ptrs, n_layers, width, height, views=False):
        """dev_ptrs: flat list of n_segments*n_layers device pointers."""
        ptrs = (C.c_void_p * len(dev_ptrs))(*[int(p) for p in dev_ptrs])
        return self._run_tex_batch(self.L.uvol_encode_texture_segments_dev, ptrs, len(dev_ptrs) // n_layers, n_layers, width, height, views)

    def encode_texture_segments_status(self, segments, caps=None):
        """Per-segment results (uvol_encode_texture_segments_st): -> (list of .ktx2 bytes or None, list of status codes).  caps: optional
        output capacities per segment (tests: a too-small one fails alone with UVOL_E_NOSPACE)."""
        flat, ptrs, w, h, nl, nseg = _segments(segments)
        run = lambda outs, capa, lens, st: self.L.uvol_encode_texture_segments_st(self.h, ptrs, nseg, nl, w, h, 0, outs, capa, lens, st)
        return self._run_tex_st(run, "encode_texture_segments_st", nseg, self.L.uvol_texture_bound(w, h, nl), caps)

    def _run_tex_st(self, run, name, nseg, cap, caps):
        """The per-segment texture encode forms: fresh output buffers of `cap` bytes (or the caller's `caps`) -> (list of .ktx2 bytes or None,
        list of status codes)."""
        cl = [cap] * nseg if caps is None else [int(c) for c in caps]
        bufs = [np.empty(max(c, 1), dtype=np.uint8) for c in cl]
        outs = (C.c_void_p * nseg)(*[b.ctypes.data for b in bufs]); capa = (C.c_size_t * nseg)(*cl); lens = (C.c_size_t * nseg)(); st = (C.c_int * nseg)()
        rc = run(outs, capa, lens, st)
        if rc != UVOL_OK:
            raise UvolError(f"{name} rc={rc}: {self.error()}")
        return [bufs[i][:lens[i]].tobytes() if st[i] == UVOL_OK else None for i in range(nseg)], list(st)

    def encode_texture_segments_mips(self, segments, levels=0, caps=None, dev_ptrs=None, shape=None):
        """uvol_encode_texture_segments_mips: every segment -> ONE .ktx2 with `levels` mip levels (0: the full chain; a UASTC context) ->
        (list of .ktx2 bytes or None, list of status codes).  segments: lists of HxWx4 uint8 arrays; or dev_ptrs = a flat list of
        n_segments * n_layers device pointers with shape = (width, height, n_layers).  caps: optional output capacities per segment."""
        if dev_ptrs is not None:
            w, h, nl = shape; flat = [int(p) for p in dev_ptrs]; nseg = len(flat) // nl
            ptrs = (C.c_void_p * len(flat))(*flat)
        else:
            flat, ptrs, w, h, nl, nseg = _segments(segments)
        run = lambda outs, capa, lens, st: self.L.uvol_encode_texture_segments_mips(self.h, ptrs, nseg, nl, w, h, 0 if dev_ptrs is None else 1, levels, outs, capa, lens, st)
        return self._run_tex_st(run, "encode_texture_segments_mips", nseg, self.L.uvol_texture_bound_mips(w, h, nl, levels) or self.L.uvol_texture_bound(w, h, nl), caps)

    def ktx2_levels(self, data: bytes):
        """uvol_ktx2_levels: the mip level count of a .ktx2 this codec reads (1 for an ETC1S file)."""
        n = C.c_uint32()
        rc = self.L.uvol_ktx2_levels(data, len(data), C.byref(n))
        if rc != UVOL_OK:
            raise UvolError(f"uvol_ktx2_levels rc={rc}")
        return n.value

    TARGETS = {"rgba32": (0, 4, False), "etc1": (1, 8, True), "bc7": (2, 16, True), "astc": (3, 16, True), "etc2_rgba": (4, 16, True), "bc1": (5, 8, True), "bc3": (6, 16, True)}

    def transcode_texture_segments_status(self, files, target="rgba32", shape=None, level=None):
        """Per-segment results and mixed batches (uvol_transcode_texture_segments_st): files may mix ETC1S and UASTC sources and contain
        unreadable or corrupt ones -> (list of arrays or None, list of status codes).  shape = (w, h, layers) if the first file is not readable.
        level: the mip level asked of every file (uvol_transcode_texture_segments_level): the arrays have the LEVEL's size; shape stays the
        files' level-0 shape."""
        files, fp, ln, n = _files(files); st = (C.c_int * n)()
        code, unit, blocks = self.TARGETS[target]
        if shape is None:
            for f in files:
                try:
                    shape = self.ktx2_info(f); break
                except UvolError:
                    continue
        w, h, nl = shape
        if level is not None:
            w, h = max(1, w >> level), max(1, h >> level)
        bx, by = (w + 3) // 4, (h + 3) // 4
        outs = [np.zeros((nl, by, bx, unit) if blocks else (nl, h, w, 4), dtype=np.uint8) for _ in range(n)]
        ptrs = (C.c_void_p * (n * nl))(*[outs[s][l].ctypes.data for s in range(n) for l in range(nl)])
        if level is None:
            rc = self.L.uvol_transcode_texture_segments_st(self.h, fp, ln, n, ptrs, bx * by * unit if blocks else w * h * 4, 0, code, st)
        else:
            rc = self.L.uvol_transcode_texture_segments_level(self.h, fp, ln, n, level, ptrs, bx * by * unit if blocks else w * h * 4, code, 0, st)
        if rc != UVOL_OK:
            raise UvolError(f"transcode_texture_segments_st rc={rc}: {self.error()}")
        return [outs[i] if st[i] == UVOL_OK else None for i in range(n)], list(st)

    def _run_tex_batch(self, fn, ptrs, nseg, nl, w, h, views=False):
        bufs, outs, caps = self._slot_bufs(("tex", "blocking"), nseg, cap=self.L.uvol_texture_bound(w, h, nl)); lens = (C.c_size_t * nseg)()
        rc = fn(self.h, ptrs, nseg, nl, w, h, outs, caps, lens)
        if rc != UVOL_OK:
            raise UvolError(f"encode_texture_segments rc={rc}: {self.error()}")
        return [(bufs[i][:lens[i]] if views else bufs[i][:lens[i]].tobytes()) for i in range(nseg)]

    def _run_tex(self, fn, ptrs, n, w, h):
        cap = self.L.uvol_texture_bound(w, h, n)
        out = np.empty(cap, dtype=np.uint8); ln = C.c_size_t()
        rc = fn(self.h, ptrs, n, w, h, out.ctypes.data, cap, C.byref(ln))
        if rc != UVOL_OK:
            raise UvolError(f"encode_texture_segment rc={rc}: {self.error()}")
        return out[:ln.value].tobytes()

    # ---- decode path (texture half) ----
    def ktx2_info(self, data: bytes):
        w, h, n = C.c_uint32(), C.c_uint32(), C.c_uint32()
        rc = self.L.uvol_ktx2_info(data, len(data), C.byref(w), C.byref(h), C.byref(n))
        if rc != UVOL_OK:
            raise UvolError(f"uvol_ktx2_info rc={rc}")
        return w.value, h.value, n.value

    def decode_texture_segments(self, files, out=None):
        """files: list of .ktx2 bytes (one width / height / layer count) -> list (per segment) of [layers, H, W, 4] uint8 arrays,
        rows in stored order (the encoder's -y_flip is part of the stored image)."""
        files, fp, ln, n = _files(files)
        w, h, nl = self.ktx2_info(files[0])
        outs = out if out is not None else [np.empty((nl, h, w, 4), dtype=np.uint8) for _ in range(n)]      # out: arrays of an earlier call, re-used
        ptrs = (C.c_void_p * (n * nl))(*[outs[s][l].ctypes.data for s in range(n) for l in range(nl)])
        rc = self.L.uvol_decode_texture_segments(self.h, fp, ln, n, ptrs, w * h * 4)
        if rc != UVOL_OK:
            raise UvolError(f"decode_texture_segments rc={rc}: {self.error()}")
        return outs

    def _transcode(self, files, entry, unit, name):
        """The single-target transcode methods: -> list (per segment) of [layers, by, bx, unit] uint8 arrays of 4x4 blocks (raster order)."""
        files, fp, ln, n = _files(files)
        w, h, nl = self.ktx2_info(files[0]); bx, by = (w + 3) // 4, (h + 3) // 4
        outs = [np.empty((nl, by, bx, unit), dtype=np.uint8) for _ in range(n)]
        ptrs = (C.c_void_p * (n * nl))(*[outs[s][l].ctypes.data for s in range(n) for l in range(nl)])
        rc = entry(self.h, fp, ln, n, ptrs, bx * by * unit, 0)
        if rc != UVOL_OK:
            raise UvolError(f"{name} rc={rc}: {self.error()}")
        return outs

    def transcode_texture_segments_etc1(self, files):
        """files: list of .ktx2 bytes -> list (per segment) of [layers, by, bx, 8] uint8 arrays of ETC1 blocks (raster order)."""
        return self._transcode(files, self.L.uvol_transcode_texture_segments_etc1, 8, "transcode_texture_segments_etc1")

    def transcode_texture_segments_bc7(self, files):
        """files: list of .ktx2 bytes -> list (per segment) of [layers, by, bx, 16] uint8 arrays of BC7 mode-6 blocks (raster order)."""
        return self._transcode(files, self.L.uvol_transcode_texture_segments_bc7, 16, "transcode_texture_segments_bc7")

    def transcode_texture_segments_etc2_rgba(self, files):
        """files: list of .ktx2 bytes (with or without alpha slices) -> list (per segment) of [layers, by, bx, 16] uint8 arrays of ETC2 RGBA blocks."""
        return self._transcode(files, self.L.uvol_transcode_texture_segments_etc2_rgba, 16, "transcode_texture_segments_etc2_rgba")

    def transcode_texture_segments_astc(self, files):
        """files: list of UASTC .ktx2 bytes -> list (per segment) of [layers, by, bx, 16] uint8 arrays of ASTC 4x4 blocks (raster order)."""
        return self._transcode(files, self.L.uvol_transcode_texture_segments_astc, 16, "transcode_texture_segments_astc")

    def decode_texture_segments_dev(self, files, dev_ptrs, layer_cap):
        """Same, into caller-owned device buffers: dev_ptrs = flat list of n_segments*layers device pointers."""
        files, fp, ln, n = _files(files)
        ptrs = (C.c_void_p * len(dev_ptrs))(*[int(p) for p in dev_ptrs])
        rc = self.L.uvol_decode_texture_segments_dev(self.h, fp, ln, n, ptrs, layer_cap)
        if rc != UVOL_OK:
            raise UvolError(f"decode_texture_segments_dev rc={rc}: {self.error()}")

    # ---- decode path (geometry half) ----
    def decode_arena_bytes(self, files, materials=False):
        """Bytes of a PinnedArena that holds the output arrays of decode_mesh_batch(files, arena=...): capacities by uvol_drc_info (the counts
        are not known before the decode: 3 x faces values per attribute at most)."""
        tot = 0
        for f in files:
            nf, mv = C.c_uint32(), C.c_uint32()
            if self.L.uvol_drc_info(bytes(f), len(f), C.byref(nf), C.byref(mv)) != UVOL_OK:
                raise UvolError("not a .drc this decoder handles")
            tot += mv.value * 32 + 3 * nf.value * 12 + 6 * 256 + ((nf.value + 256) if materials else 0)      # (materials: + one id per face)
        return tot + 4096

    def decode_mesh_batch(self, files, raise_on_error=True, fetch=True, views=False, arena=None, materials=False):
        """files: list of .drc bytes -> list of dicts {pos [n,3], uv [n,2], nrm [n,3] float32 in decoding order,
        idx_pos / idx_uv / idx_nrm [3*faces] uint32 entry index per corner, face_mat [faces] uint8 material id per face}; absent attributes
        (and face_mat of a file without a GENERIC uint8 one-component vertex or corner attribute) are None.  face_mat is only there with materials=True
        (uvol_decode_mesh_batch_mat: one more kernel and one more array per frame; size an arena with decode_arena_bytes(files, materials=True)).
        arena (a PinnedArena, with views=True): the output arrays are carved from it - outputs that all lie in uvol_host_alloc memory are written
        by the DMA engines where they are, without the library's staging buffers."""
        files, fp, ln, n = _files(files); st = (C.c_int * n)()
        metas = (DecodedMesh * n)(); keep = []
        pool = self.__dict__.setdefault("_dec_bufs_pinned" if arena is not None else "_dec_bufs", []) if views else None      # views=True: the arrays are kept and re-used by the next call
        mk = (lambda shape, dt: arena.take(shape, dt)) if arena is not None else (lambda shape, dt: np.empty(shape, dt))
        for i, f in enumerate(files):
            nf, mv = C.c_uint32(), C.c_uint32()
            if self.L.uvol_drc_info(f, len(f), C.byref(nf), C.byref(mv)) != UVOL_OK:
                raise UvolError(f"frame {i}: not a .drc this decoder handles")
            a = pool[i] if (pool is not None and i < len(pool) and pool[i]["idx_pos"].size >= 3 * nf.value and pool[i]["pos"].shape[0] >= mv.value) else None
            if a is None:
                a = dict(pos=mk((mv.value, 3), np.float32), uv=mk((mv.value, 2), np.float32), nrm=mk((mv.value, 3), np.float32),
                         idx_pos=mk((3 * nf.value,), np.uint32), idx_uv=mk((3 * nf.value,), np.uint32), idx_nrm=mk((3 * nf.value,), np.uint32))
                if pool is not None:
                    if i < len(pool):
                        pool[i] = a
                    else:
                        pool.append(a)
            keep.append(a)
            m = metas[i]; m.cap_faces = nf.value; m.cap_values = mv.value
            for k, v in a.items():
                setattr(m, k, v.ctypes.data if fetch else None)        # fetch=False: decode only, results stay on the device (timing)
        fmats = None; hm = (C.c_int * n)()
        if fetch and materials:                # (with an arena the ids lie in it too: one pageable output would send the whole call through the staging buffers)
            fmats = [mk((max(1, metas[i].cap_faces),), np.uint8) for i in range(n)]
        if fmats is not None:
            fmp = (C.c_void_p * n)(*[a.ctypes.data for a in fmats])
            rc = self.L.uvol_decode_mesh_batch_mat(self.h, fp, ln, n, 0, metas, fmp, hm, st)
        else:
            rc = self.L.uvol_decode_mesh_batch(self.h, fp, ln, n, metas, st)
        if rc != UVOL_OK:
            raise UvolError(f"decode_mesh_batch rc={rc}: {self.error()}")
        res = []
        for i in range(n):
            if st[i] != UVOL_OK:
                if raise_on_error:
                    raise UvolError(f"frame {i} failed status={st[i]}: {self.error()}")
                res.append(None); continue
            m, a = metas[i], keep[i]
            cnt = dict(pos=m.n_pos, uv=m.n_uv, nrm=m.n_nrm)
            if not fetch:
                res.append(dict(n_faces=m.n_faces, n_pos=m.n_pos, n_uv=m.n_uv, n_nrm=m.n_nrm)); continue
            cp = (lambda v: v) if views else (lambda v: v.copy())
            res.append({k: (cp(a[k][:cnt[k]]) if cnt[k] else None) for k in ("pos", "uv", "nrm")} |
                       {"idx_" + k: (cp(a["idx_" + k][:3 * m.n_faces]) if cnt[k] else None) for k in ("pos", "uv", "nrm")} | {"n_faces": m.n_faces} |
                       ({"face_mat": (cp(fmats[i][:m.n_faces]) if hm[i] else None)} if fmats is not None else {}))
        return res

    def points_arena_bytes(self, files):
        """Bytes of a PinnedArena that holds the output arrays of decode_mesh_batch_points(files, arena=...), either layout."""
        tot = 0
        for f in files:
            nf, mv = self.drc_info(f)
            tot += mv * 32 + 3 * nf * 4 + 4 * 256
        return tot + 4096

    def decode_mesh_batch_points(self, files, layout="planar", on_device=False, arena=None, raise_on_error=True, metas=None, status_out=None):
        """files: list of .drc bytes -> per frame the render-ready form (uvol_decode_mesh_batch_points): a dict {index [3*faces] uint32 point per
        corner, n_faces, n_points, has_uv, has_nrm} plus, layout="planar", pos [n,3] / uv [n,2] / nrm [n,3] float32 (None for an attribute the
        file does not carry) or, layout="interleaved", points [n,8] float32 = pos[3] nrm[3] uv[2] (absent slots zero).  Points are numbered by
        first appearance in corner order.  arena (a PinnedArena): the arrays are views into it, written by DMA where they lie.
        on_device=True: `metas` is a (DecodedPoints * n) array whose pointers are DEVICE memory of the caller (capacities by drc_info); the
        arrays stay in HBM and the call returns the statuses, the counts are in `metas`.  A failed frame is None (raise_on_error=False); a
        foreign file or a frame that does not fit fails alone.  status_out (a list): receives the per-frame codes of a host-output call; with
        `metas` (capacities of the caller's choosing, arrays allocated here) n_points / n_faces of a frame that did not fit are the needed counts."""
        lay = {"planar": UVOL_POINTS_PLANAR, "interleaved": UVOL_POINTS_INTERLEAVED}[layout]
        if on_device and metas is not None:
            for m in metas:
                m.layout = lay

        def attach(m, cp, cf, mk):
            m.layout = lay
            a = dict(index=mk((3 * cf,), np.uint32))
            if lay == UVOL_POINTS_INTERLEAVED:
                a["points"] = mk((cp, 8), np.float32); m.pos = a["points"].ctypes.data; m.uv = None; m.nrm = None
            else:
                a["pos"] = mk((cp, 3), np.float32); a["uv"] = mk((cp, 2), np.float32); a["nrm"] = mk((cp, 3), np.float32)
                m.pos, m.uv, m.nrm = a["pos"].ctypes.data, a["uv"].ctypes.data, a["nrm"].ctypes.data
            m.index = a["index"].ctypes.data
            return a

        def result(m, a):
            npnt = m.n_points
            r = dict(index=a["index"][:3 * m.n_faces], n_faces=m.n_faces, n_points=npnt, has_uv=bool(m.has_uv), has_nrm=bool(m.has_nrm))
            if lay == UVOL_POINTS_INTERLEAVED:
                r["points"] = a["points"][:npnt]
            else:
                r["pos"] = a["pos"][:npnt]; r["uv"] = a["uv"][:npnt] if m.has_uv else None; r["nrm"] = a["nrm"][:npnt] if m.has_nrm else None
            return r
        return self._decode_welded("decode_mesh_batch_points", self.L.uvol_decode_mesh_batch_points, DecodedPoints, attach, result,
                                   files, on_device, arena, raise_on_error, metas, status_out)

    def _decode_welded(self, name, entry, struct, attach, result, files, on_device, arena, raise_on_error, metas, status_out):
        """The render-ready decode methods.  attach(m, cap_points, cap_faces, mk) allocates one frame's output arrays with mk(shape, dtype) and
        sets m's pointers -> the arrays; result(m, arrays) is a decoded frame's dict."""
        files, fp, ln, n = _files(files); st = (C.c_int * n)()
        if on_device:
            if metas is None:
                raise UvolError(f"{name}(on_device=True) takes the caller's device buffers in `metas`")
            rc = entry(self.h, fp, ln, n, 1, metas, st)
            if rc != UVOL_OK:
                raise UvolError(f"{name} rc={rc}: {self.error()}")
            return list(st)
        own = metas is None
        if own:
            metas = (struct * n)()
        mk = (lambda shape, dt: arena.take(shape, dt)) if arena is not None else (lambda shape, dt: np.empty(shape, dt))
        keep = []
        for i, f in enumerate(files):
            m = metas[i]
            if own:
                nf, mv = C.c_uint32(), C.c_uint32()
                ok = self.L.uvol_drc_info(f, len(f), C.byref(nf), C.byref(mv)) == UVOL_OK      # (a foreign file fails in its own slot below)
                m.cap_faces = nf.value if ok else 0; m.cap_points = mv.value if ok else 0
            keep.append(attach(m, max(1, int(m.cap_points)), max(1, int(m.cap_faces)), mk))
        rc = entry(self.h, fp, ln, n, 0, metas, st)
        if status_out is not None:
            status_out[:] = list(st)
        if rc != UVOL_OK:
            raise UvolError(f"{name} rc={rc}: {self.error()}")
        res = []
        for i in range(n):
            if st[i] != UVOL_OK:
                if raise_on_error:
                    raise UvolError(f"frame {i} failed status={st[i]}: {self.error()}")
                res.append(None); continue
            res.append(result(metas[i], keep[i]))
        return res

    def decode_mesh_batch_packed(self, files, on_device=False, arena=None, raise_on_error=True, metas=None, status_out=None):
        """files: list of .drc bytes -> per frame the packed render-ready form (uvol_decode_mesh_batch_packed): a dict {records [n] PACKED_RECORD
        (uint16 pos[3], uint16 material, uint16 uv[2], int8 nrm[4]: the file's quantised integers, the normal times 127 rounded), index
        [3*faces] uint32 point per corner, n_faces, n_points, has_uv, has_nrm, has_material, pos_bits, uv_bits, pos_min [3], pos_scale, uv_min
        [2], uv_scale (float32: value = min + q * scale, product rounded before the sum)}.  Points and index are those of
        decode_mesh_batch_points, except in a frame whose material is a corner attribute (interior material seams): there the corner's material
        is part of the point tuple, and a point shared by two materials becomes one point per material.  The other arguments are those of decode_mesh_batch_points, `metas` a (PackedPoints * n) array; a
        PinnedArena of points_arena_bytes(files) is large enough."""
        def attach(m, cp, cf, mk):
            a = dict(index=mk((3 * cf,), np.uint32), records=mk((cp, 16), np.uint8))
            m.records = a["records"].ctypes.data; m.index = a["index"].ctypes.data
            return a
        result = lambda m, a: dict(packed_meta(m), index=a["index"][:3 * m.n_faces], records=a["records"][:m.n_points].view(PACKED_RECORD).reshape(-1))
        return self._decode_welded("decode_mesh_batch_packed", self.L.uvol_decode_mesh_batch_packed, PackedPoints, attach, result,
                                   files, on_device, arena, raise_on_error, metas, status_out)

    # ---- measurement ----
    def profile(self, on=True):
        self.L.uvol_profile_enable(self.h, 1 if on else 0)

    def profile_reset(self):
        self.L.uvol_profile_reset(self.h)

    def profile_report(self):
        self.L.uvol_sync(self.h)
        out = []
        for i in range(self.L.uvol_profile_count(self.h)):
            name = C.create_string_buffer(128); la = C.c_uint64(); ms = C.c_double(); ab = C.c_uint64()
            self.L.uvol_profile_get(self.h, i, name, 128, C.byref(la), C.byref(ms), C.byref(ab))
            out.append(dict(name=name.value.decode(), launches=la.value, total_ms=ms.value, algo_bytes=ab.value))
        return out
