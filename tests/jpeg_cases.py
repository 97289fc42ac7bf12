"""Checks of the JPEG ingest (host/uvol_host.cpp read_jpeg_raw / read_jpeg, uvol_idct_jpeg_batch_dev in csrc/jpeg_ingest.hip), shared by
tests/test_hipemu_jpeg.py (the host emulation of the kernels, no GPU) and tests/test_gpu_jpeg.py (the MI355X).  `mem` is material_cases.HostMem /
HipMem: how "device" memory is read back.

The reference is the restatement below of the decoding rule as include/uvol_codec.h states it, written from that text: a plain-Python marker
parse and Huffman decode, and the rest in NumPy.
  F[v][u] = clamp(coef q, -32768, 32767);  K[x][u] = floor(8192 s_u cos((2 x + 1) u pi / 16) + 0.5), s_0 = 1 / (2 sqrt 2), s_u = 1 / 2
  b[y][u] = clamp((sum_v K[y][v] F[v][u] + 1024) >> 11, -32768, 32767);  p[y][x] = (sum_u K[x][u] b[y][u] + 16384) >> 15;  clamp(p + 128, 0, 255)
  chroma over its REAL extent ceil(W h_c / hmax) x ceil(H v_c / vmax) (a neighbour outside it is the sample itself):
    2 x 1: out[2 i] = (3 c + l + 1) >> 2, out[2 i + 1] = (3 c + r + 2) >> 2
    2 x 2: a_even = 3 c + above, a_odd = 3 c + below (not rounded), then out[2 i] = (3 a + a_left + 8) >> 4, out[2 i + 1] = (3 a + a_right + 7) >> 4
  R = Y + ((91881 cr + 32768) >> 16), G = Y - ((22554 cb + 46802 cr + 32768) >> 16), B = Y + ((116130 cb + 32768) >> 16), clamped; alpha 255.
Device, host reader and this restatement agree bit for bit: the only tolerance in this file is the measured closeness to libjpeg (LIBJPEG_*)."""
import ctypes as C
import os
import struct
import zlib
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden", "jpeg")
HOSTLIB = os.path.join(ROOT, "universal-volumetric_amd", "libuvolhost.so")

ACCEPTED = ("grey_1x1", "grey_8x8", "c420_16x16", "c420_17x9", "c420_47x17", "c422_24x40", "c444_33x31", "q1_420_19x13", "q100_444_20x12",
            "opt_420_24x24", "rstblk_420_33x17", "rstrow_422_40x20", "stuffed_444_24x16")
SEQUENCE = tuple("seq_%d" % k for k in range(5))             # 24 x 24, 4:2:0, a quality per frame
# status of the host reader (0: a variant the rule refuses = UVOL_E_UNSUPPORTED at the C ABI's level; -1: corrupt) and a word of its message
REFUSED = {"bad_progressive": (0, "progressive"), "bad_cmyk": (0, "four components"), "bad_luma_1x2": (0, "sampling layout 1x2"),
           "bad_truncated": (-1, "truncated"), "bad_no_dht": (-1, "Huffman table")}

# Closeness of the rule to libjpeg-turbo (Pillow 12.2), measured on the CPU over ACCEPTED + SEQUENCE against golden/jpeg/expected.npz: the
# largest channel difference is 3 levels, the lowest PSNR 53.05 dB (q1_420_19x13, quality 1).  The bound is that
# measurement plus one level and minus 1 dB: the fixture set is finite, libjpeg's IDCT is a different, equally legal rounding, and the standard
# itself allows +-1 per sample before colour conversion.
LIBJPEG_MAX_DIFF = 3 + 1
LIBJPEG_MIN_PSNR = 53.05 - 1.0


def fixture(name):
    return open(os.path.join(GOLD, name + ".jpg"), "rb").read()


# ---------------------------------------------------------------------------------------------- the restatement: Huffman decode
ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)


class Parsed:
    """w, h, ncomp, hs, vs (luma sampling), qt [ncomp, 64] uint16 (natural order), coef: flat int16 in the layout of include/uvol_codec.h"""


def parse(data):
    """Baseline JPEG -> Parsed.  For valid accepted files only (the fixtures); no error handling."""
    assert data[:2] == b"\xff\xd8"
    qt, huff, p, ri = {}, {}, 2, 0
    while True:
        while data[p] == 0xFF and data[p + 1] == 0xFF:
            p += 1
        m = data[p + 1]; L = (data[p + 2] << 8) | data[p + 3]; body = data[p + 4:p + 2 + L]; p += 2 + L
        if m == 0xDB:
            o = 0
            while o < len(body):
                assert body[o] >> 4 == 0
                t = np.zeros(64, np.uint16); t[list(ZIGZAG)] = list(body[o + 1:o + 65]); qt[body[o] & 15] = t; o += 65
        elif m == 0xC4:
            o = 0
            while o < len(body):
                counts = body[o + 1:o + 17]; n = sum(counts); syms = body[o + 17:o + 17 + n]
                table, code, k = {}, 0, 0
                for ln in range(1, 17):
                    for _ in range(counts[ln - 1]):
                        table[(ln, code)] = syms[k]; code += 1; k += 1
                    code <<= 1
                huff[(body[o] >> 4, body[o] & 15)] = table; o += 17 + n
        elif m == 0xC0:
            assert body[0] == 8
            h, w, nc = (body[1] << 8) | body[2], (body[3] << 8) | body[4], body[5]
            comps = [(body[6 + 3 * c], body[7 + 3 * c] >> 4, body[7 + 3 * c] & 15, body[8 + 3 * c]) for c in range(nc)]
        elif m == 0xDD:
            ri = (body[0] << 8) | body[1]
        elif m == 0xDA:
            assert body[0] == nc
            sel = [(body[2 + 2 * c] >> 4, body[2 + 2 * c] & 15) for c in range(nc)]
            break
    P = Parsed(); P.w, P.h, P.ncomp = w, h, nc
    if nc == 1:
        comps = [(comps[0][0], 1, 1, comps[0][3])]
    P.hs, P.vs = comps[0][1], comps[0][2]
    mw, mh = -(-w // (8 * P.hs)), -(-h // (8 * P.vs))
    P.qt = np.stack([qt[c[3]] for c in comps])
    grids = [np.zeros((mh * c[2], mw * c[1], 64), np.int16) for c in comps]
    # the scan's bits: stuffing removed, restart markers taken out as they come
    pos, buf, cnt = p, 0, 0

    def bit():
        nonlocal pos, buf, cnt
        if cnt == 0:
            b = data[pos]; pos += 1
            if b == 0xFF:
                assert data[pos] == 0; pos += 1
            buf, cnt = b, 8
        cnt -= 1
        return (buf >> cnt) & 1

    def symbol(table):
        code = 0
        for ln in range(1, 17):
            code = (code << 1) | bit()
            if (ln, code) in table:
                return table[(ln, code)]
        raise AssertionError("no such code")

    def value(s):
        v = 0
        for _ in range(s):
            v = (v << 1) | bit()
        return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v
    pred = [0] * nc; rst = 0
    for mcu in range(mw * mh):
        if ri and mcu and mcu % ri == 0:
            cnt = 0
            while data[pos] == 0xFF and data[pos + 1] == 0xFF:
                pos += 1
            assert data[pos] == 0xFF and data[pos + 1] == 0xD0 + rst, "restart marker"
            pos += 2; rst = (rst + 1) & 7; pred = [0] * nc
        mx, my = mcu % mw, mcu // mw
        for c, (_, hc, vc, _) in enumerate(comps):
            for v in range(vc):
                for hh in range(hc):
                    blk = grids[c][my * vc + v, mx * hc + hh]
                    s = symbol(huff[(0, sel[c][0])]); pred[c] += value(s); blk[0] = pred[c]
                    k = 1
                    while k < 64:
                        rs = symbol(huff[(1, sel[c][1])]); r, s = rs >> 4, rs & 15
                        if s == 0:
                            if r != 15:
                                break
                            k += 16; continue
                        k += r; blk[ZIGZAG[k]] = value(s); k += 1
    P.coef = np.concatenate([g.reshape(-1) for g in grids])
    return P


# ---------------------------------------------------------------------------------------------- the restatement: coefficients -> RGBA
def cos_table():
    x = np.arange(8, dtype=np.float64)[:, None]; u = np.arange(8, dtype=np.float64)[None, :]
    s = np.where(u == 0, 1.0 / (2.0 * np.sqrt(2.0)), 0.5)
    return np.floor(8192.0 * s * np.cos((2 * x + 1) * u * np.pi / 16.0) + 0.5).astype(np.int64)


K = cos_table()


def geometry(w, h, ncomp, hs, vs):
    """per component: (blocks wide, blocks high, real width, real height)"""
    mw, mh = -(-w // (8 * hs)), -(-h // (8 * vs))
    out = []
    for c in range(ncomp):
        hc, vc = (hs, vs) if c == 0 else (1, 1)
        out.append((mw * hc, mh * vc, -(-w * hc // hs), -(-h * vc // vs)))
    return out


def coeff_count(w, h, ncomp, hs, vs):
    return sum(bw * bh for bw, bh, _, _ in geometry(w, h, ncomp, hs, vs)) * 64


def decode(w, h, ncomp, hs, vs, coef, qt):
    """coef: flat int16 (the layout of include/uvol_codec.h), qt [ncomp, 64] -> RGBA [h, w, 4] uint8, by the rule."""
    coef = np.asarray(coef, np.int64); qt = np.asarray(qt, np.int64).reshape(ncomp, 64)
    planes, off = [], 0
    for c, (bw, bh, cw, ch) in enumerate(geometry(w, h, ncomp, hs, vs)):
        blk = coef[off:off + bw * bh * 64].reshape(bh, bw, 8, 8); off += bw * bh * 64               # [.., v, u]
        F = np.clip(blk * qt[c].reshape(8, 8), -32768, 32767)
        b = np.clip((np.einsum("yv,abvu->abyu", K, F) + 1024) >> 11, -32768, 32767)
        p = (np.einsum("xu,abyu->abyx", K, b) + 16384) >> 15
        s = np.clip(p + 128, 0, 255)
        planes.append(s.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)[:ch, :cw])
    Y = planes[0][:h, :w]
    out = np.empty((h, w, 4), np.uint8); out[..., 3] = 255
    if ncomp == 1:
        out[..., :3] = Y[..., None]; return out
    up = []
    for Cp in planes[1:]:
        if hs == 1:
            U = Cp
        elif vs == 1:
            l = np.concatenate([Cp[:, :1], Cp[:, :-1]], 1); r = np.concatenate([Cp[:, 1:], Cp[:, -1:]], 1)
            U = np.empty((Cp.shape[0], 2 * Cp.shape[1]), np.int64); U[:, 0::2] = (3 * Cp + l + 1) >> 2; U[:, 1::2] = (3 * Cp + r + 2) >> 2
        else:
            above = np.concatenate([Cp[:1], Cp[:-1]], 0); below = np.concatenate([Cp[1:], Cp[-1:]], 0)
            A = np.empty((2 * Cp.shape[0], Cp.shape[1]), np.int64); A[0::2] = 3 * Cp + above; A[1::2] = 3 * Cp + below
            l = np.concatenate([A[:, :1], A[:, :-1]], 1); r = np.concatenate([A[:, 1:], A[:, -1:]], 1)
            U = np.empty((A.shape[0], 2 * A.shape[1]), np.int64); U[:, 0::2] = (3 * A + l + 8) >> 4; U[:, 1::2] = (3 * A + r + 7) >> 4
        up.append(U[:h, :w])
    cb, cr = up[0] - 128, up[1] - 128
    out[..., 0] = np.clip(Y + ((91881 * cr + 32768) >> 16), 0, 255)
    out[..., 1] = np.clip(Y - ((22554 * cb + 46802 * cr + 32768) >> 16), 0, 255)
    out[..., 2] = np.clip(Y + ((116130 * cb + 32768) >> 16), 0, 255)
    return out


_cache = {}


def reference(name):
    """(Parsed, RGBA by the rule) of a fixture: computed once, shared, never written to."""
    if name not in _cache:
        P = parse(fixture(name)); img = decode(P.w, P.h, P.ncomp, P.hs, P.vs, P.coef, P.qt)
        img.setflags(write=False); P.coef.setflags(write=False); P.qt.setflags(write=False)
        _cache[name] = (P, img)
    return _cache[name]


# ---------------------------------------------------------------------------------------------- the host reader's C surface
def hostlib():
    L = C.CDLL(HOSTLIB)
    L.uvolh_jpeg_layout.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_uint), C.c_char_p, C.c_size_t]
    L.uvolh_jpeg_coeffs.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t]
    L.uvolh_jpeg_decode_rgba.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t]
    return L


def host_layout(L, data):
    out = (C.c_uint * 5)(); err = C.create_string_buffer(512)
    return L.uvolh_jpeg_layout(data, len(data), out, err, 512), tuple(out), err.value.decode()


def host_coeffs(L, data):
    rc, (w, h, nc, hs, vs), msg = host_layout(L, data); assert rc == 1, msg
    coef = np.zeros(coeff_count(w, h, nc, hs, vs), np.int16); qt = np.zeros((nc, 64), np.uint16); err = C.create_string_buffer(512)
    assert L.uvolh_jpeg_coeffs(data, len(data), coef.ctypes.data, coef.size, qt.ctypes.data, qt.size, err, 512) == 1, err.value
    return (w, h, nc, hs, vs), coef, qt


def host_rgba(L, data):
    rc, (w, h, nc, hs, vs), msg = host_layout(L, data); assert rc == 1, msg
    img = np.zeros((h, w, 4), np.uint8); err = C.create_string_buffer(512)
    assert L.uvolh_jpeg_decode_rgba(data, len(data), img.ctypes.data, img.size, err, 512) == 1, err.value
    return img


# ---------------------------------------------------------------------------------------------- 1. host coefficients (CPU only)
def run_host(L):
    for name in ACCEPTED + SEQUENCE:
        P, want = reference(name); data = fixture(name)
        lay, coef, qt = host_coeffs(L, data)
        assert lay == (P.w, P.h, P.ncomp, P.hs, P.vs), (name, lay)
        assert np.array_equal(qt, P.qt), name
        assert np.array_equal(coef, P.coef), (name, np.flatnonzero(coef != P.coef)[:4].tolist())
        got = host_rgba(L, data)
        assert np.array_equal(got, want), (name, np.argwhere(got != want)[:4].tolist())
    data = fixture("stuffed_444_24x16")
    assert b"\xff\x00" in data[data.index(b"\xff\xda"):]      # the fixture does hold a stuffed byte in its entropy data
    assert reference("q1_420_19x13")[0].qt.max() == 255 and reference("q100_444_20x12")[0].qt.max() == 1


# ---------------------------------------------------------------------------------------------- 2. device bit-exactness
def read_layers(mem, ptrs, w, h):
    return [mem.to_host(p, np.uint8, w * h * 4).reshape(h, w, 4) for p in ptrs]


def run_device_fixtures(cd, mem, L, arena=None):
    """Every accepted fixture as a batch of 1 (slots in turn) = the rule = the host reader.  arena: a uvol.PinnedArena - the inputs then lie in
    uvol_host_alloc memory and take the upload that skips the staging copy."""
    for k, name in enumerate(ACCEPTED):
        P, want = reference(name)
        coef, qt = (arena.put(P.coef), arena.put(P.qt)) if arena else (P.coef, P.qt)
        assert cd.jpeg_coeff_count(P.w, P.h, P.ncomp, P.hs, P.vs) == P.coef.size, name
        out = cd.idct_jpeg_batch_dev([coef], [qt], P.w, P.h, P.ncomp, P.hs, P.vs, slot=k & 1)
        got = read_layers(mem, out, P.w, P.h)[0]
        assert np.array_equal(got, want), (name, np.argwhere(got != want)[:4].tolist())
        assert np.array_equal(got, host_rgba(L, fixture(name))), name


def run_device_batch(cd, mem, arena=None):
    """The five frames of the sequence in one call, each with its own tables; both slots; the second slot's call leaves the first one's layers."""
    refs = [reference(n) for n in SEQUENCE]; P0 = refs[0][0]
    assert len({r[0].qt.tobytes() for r in refs}) == 5              # a table set per image
    put = (lambda a: arena.put(a)) if arena else (lambda a: a)
    outs = []
    for slot in (0, 1):
        order = refs if slot == 0 else refs[::-1]
        outs.append((order, cd.idct_jpeg_batch_dev([put(r[0].coef) for r in order], [put(r[0].qt) for r in order], P0.w, P0.h, 3, 2, 2, slot=slot, sync=False)))
    assert cd.L.uvol_sync(cd.h) == 0, cd.error()
    for order, ptrs in outs:
        assert ptrs[1] - ptrs[0] == P0.w * P0.h * 4
        for k, g in enumerate(read_layers(mem, ptrs, P0.w, P0.h)):
            assert np.array_equal(g, order[k][1]), (k, np.argwhere(g != order[k][1])[:4].tolist())


# ---------------------------------------------------------------------------------------------- 3. arithmetic edges
def edge_blocks():
    """(coef [n, 64], q) sets of synthetic blocks: every single coefficient at +-1 and +-2047 with q = 1 and q = 255; all 64 at +-32767 with
    q = 255 (both clamps act); a DC sweep."""
    sets = []
    for q in (1, 255):
        for v in (1, -1, 2047, -2047):
            b = np.zeros((64, 64), np.int16); b[np.arange(64), np.arange(64)] = v; sets.append((b, q))
    for v in (32767, -32767):
        sets.append((np.full((1, 64), v, np.int16), 255))
    alt = np.full((2, 64), 32767, np.int16); alt[0, 1::2] = -32767; alt[1, ::2] = -32767; sets.append((alt, 255))
    dc = np.zeros((4096, 64), np.int16); dc[:, 0] = np.linspace(-32768, 32767, 4096).astype(np.int16); sets.append((dc, 1))
    dc2 = np.zeros((512, 64), np.int16); dc2[:, 0] = np.arange(-256, 256); sets.append((dc2, 8))
    return sets


def run_arithmetic_edges(cd, mem):
    """16 x 16 at 4:2:0 (six blocks per image: the upsampler sees the values too); each set's blocks fill images six at a time, one call per set."""
    for blocks, q in edge_blocks():
        n = -(-len(blocks) // 6)
        coef = np.zeros((n, 6, 64), np.int16); coef.reshape(-1, 64)[:len(blocks)] = blocks
        qt = np.full((3, 64), q, np.uint16)
        out = cd.idct_jpeg_batch_dev(list(coef), [qt] * n, 16, 16, 3, 2, 2)
        got = read_layers(mem, out, 16, 16)
        for i in range(n):
            want = decode(16, 16, 3, 2, 2, coef[i].reshape(-1), qt)
            assert np.array_equal(got[i], want), (q, int(blocks[0].max()), i, np.argwhere(got[i] != want)[:4].tolist())
    # DC only, in closed form: a luma block of DC value F is the constant clamp(((2896 ((2896 F + 1024) >> 11) + 16384) >> 15) + 128), and with
    # chroma at 128 (all-zero blocks) the texel is that grey
    F = np.arange(-2048, 2048, 7, dtype=np.int64) * 16
    F = np.clip(F, -32768, 32767)
    n = -(-len(F) // 4)
    lum = np.zeros(n * 4, np.int64); lum[:len(F)] = F
    coef = np.zeros((n, 6, 64), np.int16); coef[:, :4, 0] = lum.reshape(n, 4)
    out = cd.idct_jpeg_batch_dev(list(coef), [np.ones((3, 64), np.uint16)] * n, 16, 16, 3, 2, 2, slot=1)
    got = read_layers(mem, out, 16, 16)
    want = np.clip(((2896 * ((2896 * lum + 1024) >> 11) + 16384) >> 15) + 128, 0, 255).reshape(n, 2, 2)
    for i in range(n):
        for by in range(2):
            for bx in range(2):
                t = got[i][8 * by:8 * by + 8, 8 * bx:8 * bx + 8]
                assert (t[..., :3] == want[i, by, bx]).all() and (t[..., 3] == 255).all(), (i, by, bx)


# ---------------------------------------------------------------------------------------------- 4. closeness to libjpeg (CPU only)
def psnr(a, b):
    d = a.astype(np.float64) - b.astype(np.float64); m = float((d * d).mean())
    return 99.0 if m == 0 else 10.0 * np.log10(255.0 * 255.0 / m)


def measure_libjpeg():
    exp = np.load(os.path.join(GOLD, "expected.npz"))
    worst, low = 0, 99.0
    for name in ACCEPTED + SEQUENCE:
        got = reference(name)[1][..., :3]; want = exp[name]
        assert got.shape == want.shape, name
        d = int(np.abs(got.astype(np.int64) - want).max()); q = psnr(got, want)
        print("%-20s max |diff| %d, PSNR %.2f dB" % (name, d, q))
        worst, low = max(worst, d), min(low, q)
    return worst, low


# ---------------------------------------------------------------------------------------------- 5. into the encoders
def run_into_encoder(O, cd, mem, uastc=False):
    """The slot's device pointers handed to the encoder (ordered behind the kernels: sync=False) = the oracle encoder's bytes for the NumPy-decoded
    layers; the same through the device downscale, factor 2.  cd: a context created with uastc=1 when `uastc`."""
    import downscale_cases as DC
    refs = [reference(n) for n in SEQUENCE[:3]]; P0 = refs[0][0]; enc = O.uastc_ktx2_encode if uastc else O.ktx2_encode
    lay = cd.idct_jpeg_batch_dev([r[0].coef for r in refs], [r[0].qt for r in refs], P0.w, P0.h, 3, 2, 2, slot=1, sync=False)
    got = cd.encode_texture_segment_dev(lay, P0.w, P0.h)
    assert got == enc([r[1] for r in refs])
    lay = cd.idct_jpeg_batch_dev([r[0].coef for r in refs], [r[0].qt for r in refs], P0.w, P0.h, 3, 2, 2, slot=0, sync=False)
    small = cd.downscale_rgba_batch_dev(lay, P0.w, P0.h, 2)
    got = cd.encode_texture_segment_dev(small, P0.w // 2, P0.h // 2)
    assert got == enc([DC.downscale(r[1], 2) for r in refs])


# ---------------------------------------------------------------------------------------------- 6. refusals
def run_host_refusals(L):
    for name, (status, word) in REFUSED.items():
        rc, _, msg = host_layout(L, fixture(name))
        assert rc == status and word in msg, (name, rc, msg)
    # an SOS ahead of the SOF, and a restart marker where none belongs
    data = fixture("c420_16x16"); sof = data.index(b"\xff\xc0"); sos = data.index(b"\xff\xda")
    L0 = 2 + ((data[sof + 2] << 8) | data[sof + 3])
    rc, _, msg = host_layout(L, data[:sof] + data[sof + L0:sos] + data[sos:])
    assert rc == -1 and "SOS before SOF" in msg, msg
    data = bytearray(fixture("rstblk_420_33x17")); k = data.index(b"\xff\xd1"); data[k + 1] = 0xD3
    rc, _, msg = host_layout(L, bytes(data))
    assert rc == -1 and "restart marker" in msg, msg


def run_bad_arguments(cd, UvolError):
    """UVOL_E_INVALID (-1) with a message that names the argument, before anything runs; n <= 0 is UVOL_OK."""
    P, want = reference("c420_16x16")

    def refused(word, coeffs, qts, *lay, **kw):
        try:
            cd.idct_jpeg_batch_dev(coeffs, qts, *lay, **kw)
        except UvolError as e:
            assert "rc=-1" in str(e) and word in str(e), (word, str(e))
            return
        raise AssertionError("not refused: " + word)
    ok = (16, 16, 3, 2, 2)
    for s in (-1, 2):
        refused("slot", [P.coef], [P.qt], *ok, slot=s)
    refused("coeffs[0]", [None], [P.qt], *ok)
    refused("qtables[1]", [P.coef, P.coef], [P.qt, None], *ok)
    refused("coeffs is NULL", None, [P.qt], *ok)
    for lay in ((16, 16, 3, 1, 2), (16, 16, 4, 1, 1), (16, 16, 2, 1, 1), (16, 16, 3, 4, 1), (0, 16, 3, 2, 2), (16, 0, 1, 1, 1), (8193, 8, 1, 1, 1), (8, 16385, 3, 2, 2)):
        refused("layout", [P.coef], [P.qt], *lay)
    assert cd.idct_jpeg_batch_dev([], [], *ok) == [] and cd.idct_jpeg_batch_dev([], [], 0, 0, 7, 9, 9, slot=5) == []
    assert cd.jpeg_coeff_count(16, 16, 3, 1, 2) == 0 and cd.jpeg_coeff_count(16, 16, 3, 2, 2) == 384
    return cd.idct_jpeg_batch_dev([P.coef], [P.qt], *ok), want


# ---------------------------------------------------------------------------------------------- 7. drivers
def write_png(path, rgba):
    """a plain 8-bit RGBA PNG (filter type 0 on every row)"""
    h, w = rgba.shape[:2]

    def chunk(t, body):
        return struct.pack(">I", len(body)) + t + body + struct.pack(">I", zlib.crc32(t + body))
    raw = b"".join(b"\x00" + rgba[y].tobytes() for y in range(h))
    open(path, "wb").write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw)) + chunk(b"IEND", b""))


def make_project(root, kinds, batch=3, corrupt=None):
    """A project of five tiny meshes and the five sequence frames; kinds[k] 'jpg' or 'png' (the NumPy-decoded frame written as a PNG, under the .jpg
    name: the drivers go by signature, not by extension); corrupt: index of a frame whose scan is cut short."""
    import json
    import cli_helpers, synth
    os.makedirs(os.path.join(root, "IMG")); os.makedirs(os.path.join(root, "OBJ"))
    for k in range(5):
        cli_helpers.write_obj(os.path.join(root, "OBJ", "frame_%05d.obj" % k), synth.sphere_mesh(16, 9, charts=(2, 2), frame=k, seed=k), short=True)
    for k, name in enumerate(SEQUENCE):
        path = os.path.join(root, "IMG", "export_%05d.jpg" % k)
        if kinds[k] == "png":
            write_png(path, reference(name)[1])
        else:
            data = fixture(name)
            open(path, "wb").write(data[:len(data) - 200] if corrupt == k else data)
    cfg = {"name": "test", "OBJFilesPath": os.path.join(root, "OBJ", "frame_#####.obj"), "ImagesPath": os.path.join(root, "IMG", "export_#####.jpg"), "KTX2_FIRST_FILE": 0, "KTX2_FILE_COUNT": 5, "KTX2_BATCH_SIZE": batch,
           "GEOMETRY_FRAME_RATE": 30, "TEXTURE_FRAME_RATE": 30, "OutputDirectory": os.path.join(root, "out")}
    p = os.path.join(root, "project-config.json"); open(p, "w").write(json.dumps(cfg, indent=1))
    return p, cfg


def segment_files(cfg, n):
    d = os.path.join(cfg["OutputDirectory"], "texture_ktx2_baseColor_default")
    assert sorted(os.listdir(d)) == ["%05d.ktx2" % s for s in range(n)]
    return [open(os.path.join(d, "%05d.ktx2" % s), "rb").read() for s in range(n)]


# (kinds per frame, flags): segments of 3, one per texture call - but for "mixed", whose two segments share one call, so that its batch holds both kinds
DRIVER_RUNS = {"dev": (["jpg"] * 5, ["--batch-frames", "3"]), "host": (["jpg"] * 5, ["--batch-frames", "3", "--host-png-unfilter"]),
               "mixed": (["png"] * 3 + ["jpg"] * 2, ["--batch-frames", "6"])}


def run_driver(O, exe, root, name):
    """`uvolenc` on the JPEG sequence (segments of 3: a short last one): every .ktx2 = the oracle encode of the NumPy-decoded frames.  name "dev":
    read_jpeg_raw + the device IDCT; "host": --host-png-unfilter (the host reader); "mixed": frames 0 - 2 PNG, 3 - 4 JPEG, decoded on the host -
    the same bytes as decoding each frame separately, since the PNGs hold the NumPy-decoded frames."""
    import subprocess
    frames = [reference(n)[1] for n in SEQUENCE]
    kinds, extra = DRIVER_RUNS[name]
    cfgp, cfg = make_project(root, kinds)
    r = subprocess.run([exe, cfgp] + extra, cwd=root, capture_output=True, text=True, timeout=900, env=dict(os.environ, UVOL_TIMING="1"))
    assert r.returncode == 0, r.stdout + r.stderr
    assert ("jpeg: marker parse + Huffman decode only" in r.stderr) == (name == "dev"), r.stderr      # which path the batches took
    assert segment_files(cfg, 2) == [O.ktx2_encode(frames[0:3]), O.ktx2_encode(frames[3:5])], name


def run_driver_corrupt_frame(O, exe, root):
    """Segments of 2, one per call: frame 2's scan is cut short, so segment 1 fails with the line of scripts/Encoder.py:293-298 and the reason;
    segment 0, encoded before it, is what it would have been."""
    import subprocess
    cfgp, cfg = make_project(root, ["jpg"] * 5, batch=2, corrupt=2)
    r = subprocess.run([exe, cfgp, "--batch-frames", "2"], cwd=root, capture_output=True, text=True, timeout=900)
    assert r.returncode == 1, r.stdout + r.stderr
    assert "Failed to compress images with indices: [2, 4]" in r.stdout and "truncated" in r.stdout, r.stdout
    assert "indices: [0, 2]" not in r.stdout
    frames = [reference(n)[1] for n in SEQUENCE]
    assert segment_files(cfg, 1) == [O.ktx2_encode(frames[0:2])]


def run_basisu_shim(O, exe, root):
    """the reference's exact command string (scripts/Encoder.py:290) with a .jpg pattern"""
    import subprocess
    cfgp, cfg = make_project(root, ["jpg"] * 5)
    pat = os.path.join(root, "IMG", "export_%05u.jpg"); out = os.path.join(root, "00000.ktx2")
    cmd = "%s -ktx2 -tex_type video -multifile_printf %s -multifile_num 3 -multifile_first 0 -y_flip -output_file %s" % (exe, pat, out)
    r = subprocess.run(cmd, shell=True, cwd=root, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    assert open(out, "rb").read() == O.ktx2_encode([reference(n)[1] for n in SEQUENCE[:3]])
