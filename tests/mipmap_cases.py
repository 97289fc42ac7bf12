"""Checks of the mip levels inside one UASTC .ktx2: the chain kernel (uvol_mipchain_rgba_batch_dev, csrc/tex_mipchain.hip), the encode
(uvol_encode_texture_segments_mips), the level-selecting read (uvol_ktx2_levels, uvol_transcode_texture_segments_level) and the drivers'
flags, shared by tests/test_hipemu_mipmaps.py (the host emulation of the kernels, no GPU) and tests/test_gpu_mipmaps.py (the MI355X).  `mem` is
material_cases.HostMem / HipMem.

The chain's reference is the NumPy restatement below of the filter as include/uvol_codec.h defines it, written from that text: level v of a
W x H image is lw x lh = max(1, W >> v) x max(1, H >> v), fx = W / lw and fy = H / lh exact; output texel (X, Y) comes in ONE step from the
n = fx fy texels of level 0 in its box:
  A = sum a, out.a = (2 A + n) // (2 n);
  per colour channel: N = sum lin[c] a, D = A (when A == 0: N = sum lin[c], D = n); m = (2 N + D) // (2 D); out.c = the v with the smallest
  |lin[v] - m|, the lower v at a tie.
For v <= 3 that is downscale_cases.downscale(img, 2 ** v), which check_restatement asserts.  The encode is pinned byte for byte against
oracle.uastc_ktx2_encode of the level-v images, the read against the existing entry points on the oracle's single-level files.
Everything is bit-exact: there is no tolerance anywhere in this file."""
import functools
import numpy as np
import downscale_cases as DC

LIN = DC.LIN
MID = LIN[:-1] + LIN[1:]          # v = how many of these lie below 2 m (an entry equal to 2 m is the tie, which goes to the lower v)


def level_count(w, h):
    return int(max(w, h)).bit_length()


def level_size(w, h, v):
    return max(1, w >> v), max(1, h >> v)


def mip(img, v):
    """img [H, W, 4] uint8 -> level v, [lh, lw, 4] uint8, in one step from level 0."""
    img = np.asarray(img); H, W = img.shape[:2]; lw, lh = level_size(W, H, v)
    assert W % lw == 0 and H % lh == 0, (W, H, v)
    fx, fy = W // lw, H // lh; n = fx * fy
    px = img.astype(np.int64)

    def box(a):
        return a.reshape((lh, fy, lw, fx) + a.shape[2:]).sum(axis=(1, 3))
    a = px[..., 3]; A = box(a)
    lin = LIN[px[..., :3]]
    Nw, Nu = box(lin * a[..., None]), box(lin)
    clear = A == 0
    N = np.where(clear[..., None], Nu, Nw); D = np.where(clear, n, A)[..., None]
    m = (2 * N + D) // (2 * D)
    out = np.empty((lh, lw, 4), np.uint8)
    out[..., :3] = np.searchsorted(MID, 2 * m, side="left")       # = argmin |lin[v] - m| with the lower v at a tie (check_restatement)
    out[..., 3] = (2 * A + n) // (2 * n)
    return out


def check_restatement():
    """CPU only: the restatement equals downscale_cases.downscale(img, 2 ** v) for v <= 3, its inverse search is the plain nearest-entry rule, and
    the worked examples of the header hold at every level."""
    rng = np.random.default_rng(41)
    m = np.arange(65536)
    assert np.array_equal(np.searchsorted(MID, 2 * m, side="left"), np.abs(LIN[None, :] - m[:, None]).argmin(-1))
    for (w, h) in ((64, 64), (96, 40), (8, 24), (256, 8)):
        img = rng.integers(0, 256, (h, w, 4)).astype(np.uint8)
        img[: h // 2, : w // 2, 3] = 0
        for v in (1, 2, 3):
            assert np.array_equal(mip(img, v), DC.downscale(img, 2 ** v)), (w, h, v)
        assert np.array_equal(mip(img, 0), img)
    const = np.empty((32, 16, 4), np.uint8); const[:] = (3, 99, 250, 17)
    for v in range(level_count(16, 32)):
        assert (mip(const, v) == const[0, 0]).all()
    assert level_count(1, 1) == 1 and level_count(4, 4) == 3 and level_count(192, 320) == 9 and level_count(8192, 16384) == 15
    assert mip(np.zeros((40, 96, 4), np.uint8), 4).shape == (2, 6, 4) and mip(np.zeros((128, 256, 4), np.uint8), 8).shape == (1, 1, 4)


# ---------------------------------------------------------------------------------------------- shared inputs and references
@functools.lru_cache(maxsize=None)
def images(w, h, n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        a = rng.integers(0, 256, (h, w, 4)).astype(np.uint8)
        a[rng.integers(0, 4, (h, w)) == 0, 3] = 0          # transparent texels among the others: the alpha-weighted branch
        a.setflags(write=False); out.append(a)
    return tuple(out)


_REF = {}


def chain_ref(img, levels):
    """Levels 1 .. levels - 1 of img, computed once per image (keyed by its bytes) and left unchanged."""
    key = (img.shape, hash(img.tobytes()))
    got = _REF.setdefault(key, {})
    for v in range(1, levels):
        if v not in got:
            got[v] = mip(img, v); got[v].setflags(write=False)
    return [got[v] for v in range(1, levels)]


def read_chain(mem, ptrs, w, h):
    """ptrs: one list per layer, entry v - 1 = level v."""
    out = []
    for lay in ptrs:
        out.append([mem.to_host(p, np.uint8, level_size(w, h, v + 1)[0] * level_size(w, h, v + 1)[1] * 4).reshape(level_size(w, h, v + 1)[1], level_size(w, h, v + 1)[0], 4)
                    for v, p in enumerate(lay)])
    return out


def check_chain(got, imgs, levels, what):
    assert len(got) == len(imgs)
    for k, (g, a) in enumerate(zip(got, imgs)):
        want = chain_ref(a, levels)
        assert len(g) == levels - 1, (what, k, len(g))
        for v, (gv, wv) in enumerate(zip(g, want), start=1):
            assert gv.shape == wv.shape and np.array_equal(gv, wv), (what, "layer", k, "level", v, np.argwhere(gv != wv)[:4].tolist())


def run_device(cd, mem, imgs, levels=0, slot=0):
    h, w = imgs[0].shape[:2]
    nl = levels or level_count(w, h)
    out = cd.mipchain_rgba_batch_dev([mem.to_dev(a) for a in imgs], w, h, levels, slot=slot)
    got = read_chain(mem, out, w, h)
    mem.free_all()
    return got, nl


# ---------------------------------------------------------------------------------------------- 1. the chain, bit-exact
# W, H, levels (0 = full).  The first six are the issue's; 6 x 10 and 1 x 8 have boxes that are no powers of two from level 1 / 2 on (the levels
# are then made from per-texel sums), 96 x 40 in full has 16 x 20 boxes at level 4.
SHAPES = ((4, 4, 0), (64, 64, 0), (256, 128, 0), (96, 40, 4), (192, 320, 7), (512, 512, 0), (6, 10, 0), (1, 8, 0), (96, 40, 0), (2, 2, 2))


def run_shapes(cd, mem):
    assert cd.mip_level_count(192, 320) == 9 and cd.mip_level_count(1, 1) == 1 and cd.mip_level_count(8192, 16384) == 15
    for k, (w, h, levels) in enumerate(SHAPES):
        imgs = images(w, h, 3, 100 + k)
        got, nl = run_device(cd, mem, imgs, levels, slot=k & 1)
        assert nl == (levels or level_count(w, h))
        check_chain(got, imgs, nl, (w, h, levels))


def run_misaligned_layer(cd, mem):
    """One device layer at an address that is 4-byte aligned only."""
    w, h = 64, 64
    imgs = images(w, h, 3, 101)
    ptrs = [mem.to_dev(imgs[0]), mem.to_dev(np.concatenate([np.zeros(4, np.uint8), imgs[1].ravel()])) + 4, mem.to_dev(imgs[2])]
    assert (ptrs[1] & 15) != 0 and (ptrs[1] & 3) == 0
    out = cd.mipchain_rgba_batch_dev(ptrs, w, h)
    check_chain(read_chain(mem, out, w, h), imgs, level_count(w, h), "4-byte aligned layer")
    mem.free_all()


def run_host_inputs(cd, mem):
    w, h = 96, 40
    imgs = images(w, h, 3, 103)
    out = cd.mipchain_rgba_batch_dev(list(imgs), w, h, 4, slot=1, on_device=False)
    check_chain(read_chain(mem, out, w, h), imgs, 4, "host inputs")
    out = cd.mipchain_rgba_batch_dev([a.tobytes() for a in imgs], w, h, 4)
    check_chain(read_chain(mem, out, w, h), imgs, 4, "host inputs as bytes")


def run_ingest_slot(cd, mem, png_scanlines):
    """Three 12 x 20 images through uvol_unfilter_png_batch_dev (sync=False: the chain orders itself behind the un-filter), 3 levels."""
    rng = np.random.default_rng(6); w, h = 12, 20
    imgs = images(w, h, 3, 104)
    lay = cd.unfilter_png_batch_dev([png_scanlines(np.array(a), rng) for a in imgs], w, h, 4, slot=1, sync=False)
    out = cd.mipchain_rgba_batch_dev(lay, w, h, 3, slot=0)
    check_chain(read_chain(mem, out, w, h), imgs, 3, "ingest slot")


# ---------------------------------------------------------------------------------------------- 2. arithmetic edges (512 x 512, full chain)
def run_arithmetic_edges(cd, mem):
    w = h = 512; nl = level_count(w, h)
    full = np.full((h, w, 4), 255, np.uint8)                  # the 1 x 1 level: sum lin a = 262144 x 65535 x 255 > 2^32
    clear = np.array(images(w, h, 1, 105)[0]); clear[..., 3] = 0      # the unweighted branch at every level
    one = np.zeros((h, w, 4), np.uint8); one[..., :3] = (0, 255, 0); one[37, 411] = (200, 100, 50, 255)      # one opaque texel in a transparent image
    const = np.empty((h, w, 4), np.uint8); const[:] = (13, 77, 254, 1)
    imgs = [full, clear, one, const]
    got, _ = run_device(cd, mem, imgs)
    check_chain(got, imgs, nl, "arithmetic edges")
    assert all((g == 255).all() for g in got[0])
    assert all((g[..., 3] == 0).all() for g in got[1])
    for v, g in enumerate(got[2], start=1):                  # its colour survives to 1 x 1; alpha by the rounding rule (2 A + n) // (2 n)
        n = 4 ** v
        Y, X = 37 >> v, 411 >> v
        assert g[Y, X].tolist() == [200, 100, 50, (2 * 255 + n) // (2 * n)], (v, g[Y, X])
    assert got[2][-1].shape == (1, 1, 4) and got[2][-1][0, 0].tolist() == [200, 100, 50, 0]
    assert all((g == const[0, 0]).all() for g in got[3])


# ---------------------------------------------------------------------------------------------- 3. slots, trim, refusals
def run_slots(cd, mem):
    a = images(64, 64, 2, 106); b = images(16, 32, 3, 107); c = images(14, 10, 2, 108)
    pa = cd.mipchain_rgba_batch_dev([mem.to_dev(x) for x in a], 64, 64, slot=0)
    pb = cd.mipchain_rgba_batch_dev([mem.to_dev(x) for x in b], 16, 32, slot=1)
    pd = cd.downscale_rgba_batch_dev([mem.to_dev(x) for x in c], 14, 10, 2, slot=0)      # the downscale slots are other memory
    pe = cd.downscale_rgba_batch_dev([mem.to_dev(x) for x in c], 14, 10, 2, slot=1)
    check_chain(read_chain(mem, pb, 16, 32), b, 6, "slot 1")
    check_chain(read_chain(mem, pa, 64, 64), a, 7, "slot 0 after slot 1 and both downscale slots were written")
    DC.check_equal(DC.read_layers(mem, pd, 14, 10, 2), c, 2, "downscale slot 0 beside the chains")
    DC.check_equal(DC.read_layers(mem, pe, 14, 10, 2), c, 2, "downscale slot 1 beside the chains")
    cd.trim()                                                  # uvol_trim gives the slots back; the next call allocates again
    pa = cd.mipchain_rgba_batch_dev([mem.to_dev(x) for x in a], 64, 64, 3, slot=0)
    check_chain(read_chain(mem, pa, 64, 64), a, 3, "after uvol_trim")
    assert cd.mipchain_rgba_batch_dev([], 64, 64) == []                 # n <= 0: UVOL_OK, nothing happens
    assert cd.mipchain_rgba_batch_dev([], 0, 0, -3, slot=5) == []
    assert cd.mipchain_rgba_batch_dev([mem.to_dev(a[0])], 64, 64, 1) == [[]]      # levels == 1: UVOL_OK, nothing to make
    mem.free_all()


def run_refusals(cd, mem, UvolError):
    """Every refusal is UVOL_E_INVALID (-1) and names the argument."""
    img = np.zeros((4, 4, 4), np.uint8); p = mem.to_dev(img)
    big = mem.to_dev(np.zeros((100, 100, 4), np.uint8))

    def refused(word, *args, **kw):
        try:
            cd.mipchain_rgba_batch_dev(*args, **kw)
        except UvolError as e:
            assert "rc=-1" in str(e) and word in str(e), (word, str(e))
            return
        raise AssertionError("not refused: " + word)
    refused("level 3 of 100 x 100", [big], 100, 100, 4)              # 100 / 12 is no integer
    refused("level 3 of 100 x 100", [big], 100, 100, 0)
    refused("level 1 of 7 x 4", [p], 7, 4, 2)
    for lv in (-1, 4, 16):
        refused("levels", [p], 4, 4, lv)
    for s in (-1, 2):
        refused("slot", [p], 4, 4, 0, slot=s)
    refused("rgba[1]", [p, 0], 4, 4, 0, on_device=True)
    refused("rgba[0]", [None, img], 4, 4, 0, on_device=False)
    refused("not 4-byte aligned", [p + 2], 4, 4, 0, on_device=True)
    for (w, h) in ((0, 4), (4, 0), (8193, 1), (1, 16385)):
        refused("width", [p], w, h, 0, on_device=True)
    got = cd.mipchain_rgba_batch_dev([big], 100, 100, 3)              # exact up to level 2; the context still works
    assert [g.shape for g in read_chain(mem, got, 100, 100)[0]] == [(50, 50, 4), (25, 25, 4)]
    mem.free_all()


# ---------------------------------------------------------------------------------------------- 4. encode: the byte pin
def level_index(data):
    """(levelCount, [(byteOffset, byteLength, uncompressedByteLength)]) of a .ktx2, read from the file itself."""
    n = int.from_bytes(data[40:44], "little")
    return n, [tuple(int.from_bytes(data[80 + 24 * v + 8 * k:88 + 24 * v + 8 * k], "little") for k in range(3)) for v in range(n)]


def oracle_level(O, layers, v):
    """(the oracle's single-level file of the level-v images, its level data, its alpha flag)."""
    f = O.uastc_ktx2_encode([mip(t, v) for t in layers])
    info = O.uastc_ktx2_info(f)
    return f, f[info["level_off"]:], info["has_alpha"]


def check_mip_file(O, cd, data, layers, levels):
    """The container rules of include/uvol_codec.h and every level's bytes against the oracle encoder."""
    h, w = layers[0].shape[:2]
    assert cd.ktx2_levels(data) == levels and cd.ktx2_info(data) == (w, h, len(layers))
    n, idx = level_index(data)
    assert n == levels
    dfd_off = int.from_bytes(data[48:52], "little"); kvd_off = int.from_bytes(data[56:60], "little")
    assert dfd_off == 80 + 24 * levels and kvd_off == dfd_off + 44
    any_alpha = False; end = len(data)
    for v in range(levels):                                   # smallest level first: level 0 ends the file
        off, ln, uln = idx[v]
        lw, lh = level_size(w, h, v)
        assert off % 16 == 0 and ln == uln == len(layers) * ((lw + 3) // 4) * ((lh + 3) // 4) * 16 and off + ln == end, (v, idx[v], end)
        end = off
        _, want, alpha = oracle_level(O, layers, v)
        assert data[off:off + ln] == want, ("level", v)
        any_alpha = any_alpha or alpha
    assert (data[dfd_off + 28 + 3] & 15) == (3 if any_alpha else 0)      # the sample's channel id: RGBA when any level has a block with alpha
    return any_alpha


def encode_cases():
    import synth
    a = [np.array(t) for t in synth.texture_sequence(3, size=64, seed=5)]
    b = [np.array(x) for x in images(96, 40, 3, 109)]
    for x in b:
        x[..., 3] = 255
    c = [t.copy() for t in a]; c[1][20:30, 8:40, 3] = 90
    return (a, 0, 7, False), (b, 4, 4, False), (c, 0, 7, True)      # layers, levels argument, level count, alpha


def run_encode(O, cu, mem, UvolError, ce):
    """cu: a UASTC context; ce: an ETC1S context."""
    cases = encode_cases()
    for layers, arg, levels, alpha in cases:
        (data,), st = cu.encode_texture_segments_mips([layers], arg)
        assert st == [0]
        assert check_mip_file(O, cu, data, layers, levels) == alpha
        # device inputs = host inputs
        h, w = layers[0].shape[:2]
        (dev,), st = cu.encode_texture_segments_mips(None, arg, dev_ptrs=[mem.to_dev(t) for t in layers], shape=(w, h, len(layers)))
        assert st == [0] and dev == data
        mem.free_all()
    a, b = cases[0][0], cases[2][0]
    # levels == 1: the bytes of the existing entry point; two segments in one call; a too-small caps[s] fails its segment alone
    one, st = cu.encode_texture_segments_mips([a, b], 1)
    assert st == [0, 0] and one == cu.encode_texture_segments_status([a, b])[0] and one[0] == O.uastc_ktx2_encode(a)
    two, st = cu.encode_texture_segments_mips([a, b], 0)
    assert st == [0, 0]
    check_mip_file(O, cu, two[0], a, 7); check_mip_file(O, cu, two[1], b, 7)
    small, st = cu.encode_texture_segments_mips([a, b], 0, caps=[len(two[0]) - 1, len(two[1])])
    assert st == [-4, 0] and small[0] is None and small[1] == two[1]
    # the divisibility rule, and an ETC1S context
    for codec, args, rc, word in ((cu, ([[np.zeros((100, 100, 4), np.uint8)]], 4), -1, "level 3 of 100 x 100"), (ce, ([a], 0), -6, "mip levels are written in the UASTC mode only (DESIGN.md section 7)"),
                                  (ce, ([a], 3), -6, "UASTC mode only")):
        try:
            codec.encode_texture_segments_mips(*args)
        except UvolError as e:
            assert ("rc=%d" % rc) in str(e) and word in str(e), str(e)
        else:
            raise AssertionError("not refused: " + word)
    (e1,), st = ce.encode_texture_segments_mips([a], 1)               # levels == 1 in an ETC1S context: the existing encode
    assert st == [0] and e1 == O.ktx2_encode(a)
    return two


# ---------------------------------------------------------------------------------------------- 5. read
UASTC_TARGETS = ("rgba32", "etc1", "bc7", "astc", "etc2_rgba", "bc1", "bc3")


def zstd_supercompress_levels(ktx2, level=6):
    """A scheme-0 multi-level UASTC .ktx2 rewritten with supercompressionScheme 2: every level's data as ONE Zstandard frame made by the system's
    libzstd (None when it is not installed), stored smallest level first, byteLength = the frame, uncompressedByteLength = the level
    (tests/helpers.py zstd_supercompress, per level)."""
    import ctypes as C
    try:
        Z = C.CDLL("libzstd.so.1")
    except OSError:
        return None
    Z.ZSTD_compressBound.restype = C.c_size_t; Z.ZSTD_compressBound.argtypes = [C.c_size_t]
    Z.ZSTD_compress.restype = C.c_size_t; Z.ZSTD_compress.argtypes = [C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_int]
    Z.ZSTD_isError.restype = C.c_uint; Z.ZSTD_isError.argtypes = [C.c_size_t]
    b = bytes(ktx2); n, idx = level_index(b)
    assert int.from_bytes(b[44:48], "little") == 0
    head = bytearray(b[:min(o for o, _, _ in idx)]); head[44:48] = (2).to_bytes(4, "little")
    body = b""
    for v in reversed(range(n)):
        off, ln, _ = idx[v]; src = b[off:off + ln]
        cap = Z.ZSTD_compressBound(len(src)); buf = C.create_string_buffer(cap)
        k = Z.ZSTD_compress(buf, cap, src, len(src), level)
        assert not Z.ZSTD_isError(k)
        head[80 + 24 * v:104 + 24 * v] = (len(head) + len(body)).to_bytes(8, "little") + int(k).to_bytes(8, "little") + len(src).to_bytes(8, "little")
        body += buf.raw[:k]
    return bytes(head) + body


def run_read(O, cu, files):
    """files: the two 7-level files of run_encode (opaque, with alpha)."""
    cases = encode_cases()
    layer_sets = (cases[0][0], cases[2][0])
    shape = (64, 64, 3)
    for v in range(7):
        singles = [oracle_level(O, layers, v)[0] for layers in layer_sets]
        for target in UASTC_TARGETS:
            got, st = cu.transcode_texture_segments_status(files, target, level=v)
            want, stw = cu.transcode_texture_segments_status(singles, target)
            assert st == [0, 0] and stw == [0, 0]
            for s in range(2):
                assert got[s].shape == want[s].shape and np.array_equal(got[s], want[s]), (target, v, s)
                if target == "rgba32":
                    assert np.array_equal(got[s], O.uastc_ktx2_decode(singles[s]))
                if target == "astc":
                    assert np.array_equal(got[s], O.uastc_ktx2_decode(singles[s], "astc"))
    # the existing entry points on the mip file mean level 0
    lvl0 = [oracle_level(O, layers, 0)[0] for layers in layer_sets]
    for s in range(2):
        assert np.array_equal(cu.decode_texture_segments([files[s]])[0], O.uastc_ktx2_decode(lvl0[s]))
        assert np.array_equal(cu.transcode_texture_segments_astc([files[s]])[0], O.uastc_ktx2_decode(lvl0[s], "astc"))
    (g0, g1), st = cu.transcode_texture_segments_status(files, "bc7")
    assert st == [0, 0] and np.array_equal(g0, O.uastc_ktx2_decode(lvl0[0], "bc7"))
    # a level beyond a file's count fails that segment only (a 4-level file of the same size beside the 7-level one)
    (short,), _ = cu.encode_texture_segments_mips([layer_sets[0]], 4)
    got, st = cu.transcode_texture_segments_status([files[0], short, files[1]], "rgba32", shape=shape, level=5)
    assert st == [0, -1, 0] and got[1] is None and np.array_equal(got[2], O.uastc_ktx2_decode(oracle_level(O, layer_sets[1], 5)[0]))
    got, st = cu.transcode_texture_segments_status(files, "rgba32", shape=shape, level=7)
    assert st == [-1, -1]
    # an ETC1S file has one level
    e = O.ktx2_encode(layer_sets[0])
    assert cu.ktx2_levels(e) == 1
    got, st = cu.transcode_texture_segments_status([e], "rgba32", level=0)
    assert st == [0] and np.array_equal(got[0], cu.transcode_texture_segments_status([e], "rgba32")[0][0])
    assert cu.transcode_texture_segments_status([e], "rgba32", shape=shape, level=1)[1] == [-1]
    # a multi-level ETC1S file (stock `basisu -mipmap` without -uastc) stays UVOL_E_UNSUPPORTED (-6), and the message names it
    import ctypes as C
    e2 = e[:40] + (2).to_bytes(4, "little") + e[44:]
    buf = np.zeros((3, 64, 64, 4), np.uint8)
    rc = cu.L.uvol_decode_texture_segments(cu.h, (C.c_char_p * 1)(e2), (C.c_size_t * 1)(len(e2)), 1, (C.c_void_p * 3)(*[buf[l].ctypes.data for l in range(3)]), 64 * 64 * 4)
    assert rc == -6 and "multi-level ETC1S" in cu.error(), (rc, cu.error())
    # a truncated level index; a level whose length disagrees with its size
    f = files[0]
    for bad in (f[:80 + 24 * 3], bytes(f[:40]) + (16).to_bytes(4, "little") + f[44:]):
        _, st = cu.transcode_texture_segments_status([files[1], bad], "rgba32", shape=shape, level=0)
        assert st[0] == 0 and st[1] != 0
    for field in (88 + 24 * 2, 80 + 24 * 6, 96 + 24 * 1):         # level 2's byteLength, level 6's byteOffset beyond the file, level 1's uncompressedByteLength
        bad = bytearray(f); bad[field:field + 8] = (int.from_bytes(f[field:field + 8], "little") + (16 if field != 80 + 24 * 6 else len(f))).to_bytes(8, "little")
        _, st = cu.transcode_texture_segments_status([bytes(bad), files[1]], "rgba32", shape=shape, level=0)
        assert st[0] != 0 and st[1] == 0, field
        try:
            cu.ktx2_levels(bytes(bad))
        except Exception:
            pass
        else:
            raise AssertionError("ktx2_levels accepted a bad level index")


def run_read_zstd(O, cu, files):
    """None: no libzstd on this machine."""
    z = zstd_supercompress_levels(files[1])
    if z is None:
        return None
    assert cu.ktx2_levels(z) == 7 and cu.ktx2_info(z) == (64, 64, 3)
    for v in (0, 3, 6):
        got, st = cu.transcode_texture_segments_status([z, files[0]], "rgba32", level=v)
        want, _ = cu.transcode_texture_segments_status([files[1], files[0]], "rgba32", level=v)
        assert st == [0, 0] and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(cu.decode_texture_segments([z])[0], cu.decode_texture_segments([files[1]])[0])
    # a frame whose content size disagrees with the header is refused before anything is inflated
    n, idx = level_index(z)
    bad = bytearray(z); bad[96 + 24 * 2:104 + 24 * 2] = (idx[2][2] + 16).to_bytes(8, "little")
    assert cu.transcode_texture_segments_status([bytes(bad)], "rgba32", shape=(64, 64, 3), level=0)[1] != [0]
    return True


# ---------------------------------------------------------------------------------------------- 6. the container, read by the reference's KTX-Parse
def run_ktx_parse(O, cu, tmp_path, node, ref):
    import hashlib, json, shutil, subprocess
    layers, arg, levels, _ = encode_cases()[2]
    (data,), _ = cu.encode_texture_segments_mips([layers], arg)
    (tmp_path / "t.ktx2").write_bytes(data)
    shutil.copy(ref, tmp_path / "ktxparse.mjs")
    js = ("import { read } from './ktxparse.mjs'; import fs from 'fs'; import crypto from 'crypto';"
          "const c = read(new Uint8Array(fs.readFileSync('t.ktx2')));"
          "console.log(JSON.stringify({w: c.pixelWidth, h: c.pixelHeight, layers: c.layerCount, sc: c.supercompressionScheme, model: c.dataFormatDescriptor[0].colorModel,"
          " n: c.levels.length, len: c.levels.map(l => l.levelData.byteLength), ulen: c.levels.map(l => l.uncompressedByteLength),"
          " sha: c.levels.map(l => crypto.createHash('sha256').update(l.levelData).digest('hex')), kv: Object.keys(c.keyValue).sort()}))")
    (tmp_path / "r.mjs").write_text(js)
    r = subprocess.run([node, "--experimental-modules", "r.mjs"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-800:]
    o = json.loads(r.stdout.strip().splitlines()[-1])
    want = [oracle_level(O, layers, v)[1] for v in range(levels)]
    assert (o["w"], o["h"], o["layers"], o["sc"], o["model"], o["n"]) == (64, 64, 3, 0, 166, levels)
    assert o["len"] == [len(x) for x in want] and o["ulen"] == o["len"]
    assert o["sha"] == [hashlib.sha256(x).hexdigest() for x in want]
    assert "KTXanimData" in o["kv"]


# ---------------------------------------------------------------------------------------------- 7. drivers
def run_driver(O, cu, bin_dir, root):
    """`uvolenc --uastc --mipmaps` on a tiny project (16 x 16 PNGs, 5 frames in segments of 3: a short last segment), with a ladder rung; the
    manifest against the same run without --mipmaps; the refusal without --uastc; the basisu shim."""
    import os, subprocess
    import cli_helpers
    exe = os.path.join(bin_dir, "uvolenc")
    outs = {}
    for name, extra in (("mips", ["--mipmaps"]), ("plain", [])):
        r0 = os.path.join(root, name); os.makedirs(r0)
        cfgp, cfg, meshes, texs = cli_helpers.make_sequence(r0, n_frames=5, tex=16, batch=3)
        r = subprocess.run([exe, cfgp, "--batch-frames", "3", "--texture-ladder", "2", "--uastc"] + extra, cwd=r0, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout + r.stderr
        outs[name] = cfg["OutputDirectory"]
    out = outs["mips"]
    for s, n in enumerate([3, 2]):
        layers = texs[3 * s:3 * s + n]
        data = open(os.path.join(out, "texture_ktx2_baseColor_default", "%05d.ktx2" % s), "rb").read()
        check_mip_file(O, cu, data, layers, 5)
        rung = open(os.path.join(out, "texture_ktx2_8x8_baseColor_default", "%05d.ktx2" % s), "rb").read()
        check_mip_file(O, cu, rung, [DC.downscale(t, 2) for t in layers], 4)
        plain = open(os.path.join(outs["plain"], "texture_ktx2_baseColor_default", "%05d.ktx2" % s), "rb").read()
        assert plain == O.uastc_ktx2_encode(layers)              # without the flag every byte is as before
    names = lambda d: sorted(os.path.relpath(os.path.join(p, f), d) for p, _, fs in os.walk(d) for f in fs)
    assert names(out) == names(outs["plain"])
    assert open(os.path.join(out, "uvol.json"), "rb").read() == open(os.path.join(outs["plain"], "uvol.json"), "rb").read()
    # --mipmaps N; --mipmaps without --uastc; a size / N pair that fails the rule: a message, exit 1, no output file
    r0 = os.path.join(root, "n2"); os.makedirs(r0)
    cfgp, cfg, meshes, texs = cli_helpers.make_sequence(r0, n_frames=3, tex=16, batch=3)
    r = subprocess.run([exe, cfgp, "--batch-frames", "3", "--uastc", "--mipmaps", "2"], cwd=r0, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    check_mip_file(O, cu, open(os.path.join(cfg["OutputDirectory"], "texture_ktx2_baseColor_default", "00000.ktx2"), "rb").read(), texs, 2)
    for name, tex, extra, word in (("etc1s", 16, ["--mipmaps"], "--uastc"), ("rule", 28, ["--uastc", "--mipmaps"], "level 3 of 28 x 28")):
        r0 = os.path.join(root, name); os.makedirs(r0)
        cfgp, cfg, meshes, texs = cli_helpers.make_sequence(r0, n_frames=3, tex=tex, batch=3)
        b = subprocess.run([exe, cfgp] + extra, cwd=r0, capture_output=True, text=True, timeout=900)
        assert b.returncode == 1 and "❌" in b.stdout and word in b.stdout, (name, b.stdout)
        left = [f for p, _, fs in os.walk(cfg["OutputDirectory"]) for f in fs] if os.path.isdir(cfg["OutputDirectory"]) else []
        assert left == [], (name, left)
    # the basisu shim: -uastc -mipmap writes the chain; -mipmap alone keeps one level and says so on stderr, exit 0
    shim = os.path.join(bin_dir, "basisu")
    png = os.path.join(root, "plain", "PNG", "export_%05u.png")
    common = ["-ktx2", "-tex_type", "video", "-multifile_printf", png, "-multifile_num", "3", "-multifile_first", "0", "-y_flip"]
    o1, o2 = os.path.join(root, "shim_u.ktx2"), os.path.join(root, "shim_e.ktx2")
    r = subprocess.run([shim] + common + ["-uastc", "-mipmap", "-output_file", o1], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    _, _, _, texs = (None, None, None, __import__("synth").texture_sequence(5, size=16, seed=3))
    check_mip_file(O, cu, open(o1, "rb").read(), texs[:3], 5)
    r = subprocess.run([shim] + common + ["-mipmap", "-output_file", o2], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "one level" in r.stderr, r.stdout + r.stderr
    assert open(o2, "rb").read() == O.ktx2_encode(texs[:3])
