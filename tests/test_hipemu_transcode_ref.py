"""The re-fit transcode targets, block by block, on the host-emulation build (no GPU): ETC1S -> BC7 / ETC2 RGBA / BC1 / BC3 and
UASTC -> ETC1 / ETC2 RGBA / BC1 / BC3.  Three layers, all exact:
 (a) every block of the library equals the plain NumPy reference of the same rule (tests/transcode_ref.py), fed from the pinned decoders;
 (b) properties that do not depend on the restated rule, through the independent decoders of tests/helpers.py: index optimality, solid
     blocks, validity the decoders do not test;
 (c) the PSNR gates of tests/test_hipemu_tex.py stay as they are (quality); these layers are the statement about correctness.
The checking functions are shared with tests/test_gpu_transcode_ref.py, which runs them on the device at larger sizes.

(b) judges one block per DISTINCT source tuple when a file is large (the library's block at the tuple's first occurrence, against the
pinned decoder's texels there): a rule error shared by reference and kernel is a function of the source tuple, and (a) has already shown
every other occurrence to carry the same bytes.  Small files are judged whole, partial edge blocks included."""
import os
import numpy as np
import pytest

import transcode_ref as R
import transcode_cases as TC

WHOLE_LAYER_BLOCKS = 4096          # files up to this many blocks: layer (b) on every block, cropped like a real image


# ------------------------------------------------------------------------------------------------
# (a) byte equality
# ------------------------------------------------------------------------------------------------
def _hex(b):
    return bytes(bytearray(np.asarray(b, np.uint8).reshape(-1))).hex()


def assert_blocks_equal(name, target, got, want, describe, mask=None):
    """got / want [layers, by, bx, unit].  On a mismatch: the count, the first few (file, layer, by, bx), both blocks in hex, the block's inputs."""
    assert got.shape == want.shape, (name, target, got.shape, want.shape)
    bad = (got != want).any(-1)
    if mask is not None:
        bad &= mask
    if bad.any():
        where = np.argwhere(bad)
        lines = ["%s -> %s: %d of %d blocks differ from the reference" % (name, target, len(where), bad.size if mask is None else int(mask.sum()))]
        for l, y, x in where[:6]:
            lines.append("  (%s, layer %d, by %d, bx %d): library %s  reference %s  inputs %s" % (name, l, y, x, _hex(got[l, y, x]), _hex(want[l, y, x]), describe(l, y, x)))
        raise AssertionError("\n".join(lines))


# ------------------------------------------------------------------------------------------------
# (b) properties through the independent decoders
# ------------------------------------------------------------------------------------------------
def _sq(a, b):
    return (a.astype(np.int64) - b.astype(np.int64)) ** 2


def _blocks_of(img, hb, wb):
    """[h, w, c] -> the texels of the hb x wb blocks that lie fully inside, [hb, wb, 16, c]."""
    c = img.shape[-1]
    return img[:hb * 4, :wb * 4].reshape(hb, 4, wb, 4, c).transpose(0, 2, 1, 3, 4).reshape(hb, wb, 16, c)


def _solid(tag, dec, src, chans, tol):
    """Blocks whose 16 source texels agree in `chans` decode to one value per channel, within tol of the source."""
    h, w = src.shape[:2]; hb, wb = h // 4, w // 4
    if hb == 0 or wb == 0:
        return 0
    s = _blocks_of(src[..., chans], hb, wb).astype(np.int64); g = _blocks_of(dec[..., chans], hb, wb).astype(np.int64)
    solid = (s.max(2) == s.min(2)).all(-1)
    one = (g.max(2) == g.min(2)).all(-1)
    assert np.all(one[solid]), (tag, "a solid block decodes to several values", np.argwhere(solid & ~one)[:4].tolist())
    err = np.abs(g[:, :, 0] - s[:, :, 0])
    okay = (err <= np.asarray(tol)).all(-1)
    assert np.all(okay[solid]), (tag, "a solid block is off by more than the format's step", np.argwhere(solid & ~okay)[:4].tolist(), err[solid & ~okay][:4].tolist())
    return int(solid.sum())


def _optimal(tag, chosen, palette, src, valid=None):
    """No palette entry is strictly closer (squared error over the channels given) to the source texel than the decoded one."""
    d = _sq(chosen, src).sum(-1)
    for j, p in enumerate(palette):
        worse = _sq(p, src).sum(-1) < d
        if valid is not None:
            worse &= valid[j]
        assert not worse.any(), (tag, "palette entry %d is closer than the index chosen" % j, np.argwhere(worse)[:4].tolist())


def _with_bits(blocks, pos, n, value):
    """A copy of 16-byte blocks with the n-bit field at bit `pos` (LSB-first numbering) set to value."""
    out = blocks.copy()
    for k in range(n):
        byte, bit = (pos + k) // 8, (pos + k) % 8
        out[..., byte] = (out[..., byte] & ~np.uint8(1 << bit)) | np.uint8(((value >> k) & 1) << bit)
    return out


def props_bc7(tag, blocks, src):
    from helpers import bc7_decode_blocks
    h, w = src.shape[:2]; by, bx = blocks.shape[:2]
    dec = bc7_decode_blocks(blocks, w, h)                                     # (asserts: mode 5 or 6 only)
    b = blocks.astype(np.int64)
    lo = sum(b[..., k] << (8 * k) for k in range(8))
    m6 = (b[..., 0] & 127) == 64
    # mode 6: alpha endpoints 127 | 127 at bits 49 .. 62, p-bits at 63 and 64
    assert np.all(((lo >> 49) & 0x3fff)[m6] == 0x3fff) and np.all(((b[..., 7] >> 7) & 1)[m6] == 1) and np.all((b[..., 8] & 1)[m6] == 1), (tag, "mode 6 alpha endpoints / p-bits")
    assert np.all((b[..., 0] >> 6)[~m6] == 0), (tag, "mode 5 rotation")
    # the palette: texel 1's index field set to every value in turn (texel 0 has an implied bit), read back at texel 1
    pal16 = []
    for j in range(16):
        p5 = _with_bits(_with_bits(blocks, 67, 2, j & 3), 98, 2, j & 3); p6 = _with_bits(blocks, 68, 4, j)
        pal16.append(bc7_decode_blocks(np.where(m6[..., None], p6, p5), bx * 4, by * 4)[0::4, 1::4])
    up = lambda a: np.repeat(np.repeat(a, 4, 0), 4, 1)[:h, :w]
    valid = [up(m6 | (j < 4)) for j in range(16)]
    _optimal(tag + " colour", dec[..., :3], [up(p[..., :3]) for p in pal16], src[..., :3], valid)
    m5 = up(~m6)
    _optimal(tag + " alpha", dec[..., 3:], [up(p[..., 3:]) for p in pal16[:4]], src[..., 3:], [m5] * 4)
    _solid(tag + " colour", dec, src, [0, 1, 2], [1, 1, 1])
    _solid(tag + " alpha", dec, src, [3], [0])
    a = src[..., 3]
    assert np.all(dec[..., 3][a == 255] == 255) and np.all(dec[..., 3][a == 0] == 0), (tag, "fully opaque / transparent texels moved")


def props_bc1(tag, blocks, src, in_bc3):
    from helpers import bc1_decode_blocks
    h, w = src.shape[:2]
    dec = bc1_decode_blocks(blocks, w, h, four_colour_always=in_bc3)
    pal = []
    for j in range(4):
        p = blocks.copy(); p[..., 4:8] = 0x55 * j
        pal.append(bc1_decode_blocks(p, w, h, four_colour_always=in_bc3))
    _optimal(tag + " colour", dec[..., :3], [p[..., :3] for p in pal], src[..., :3], [p[..., 3] == 255 for p in pal])
    _solid(tag + " colour", dec, src, [0, 1, 2], [4, 2, 4])
    if not in_bc3:
        b = blocks.astype(np.int64); c0 = b[..., 0] | (b[..., 1] << 8); c1 = b[..., 2] | (b[..., 3] << 8)
        assert np.all(dec[..., 3] == 255), (tag, "a BC1 block of an opaque source decodes a transparent texel")
        assert np.all((c0 > c1) | ((c0 == c1) & (b[..., 4:8] == 0).all(-1))), (tag, "colour0 <= colour1 with indices other than 0")
    return dec


def props_bc3(tag, blocks, src):
    from helpers import bc3_decode_blocks
    h, w = src.shape[:2]
    dec = bc3_decode_blocks(blocks, w, h)
    assert np.array_equal(dec[..., :3], props_bc1(tag, blocks[..., 8:], src, True)[..., :3])
    pal = []
    for j in range(8):
        p = blocks.copy(); bits = sum(j << (3 * i) for i in range(16))
        for k in range(6):
            p[..., 2 + k] = (bits >> (8 * k)) & 255
        pal.append(bc3_decode_blocks(p, w, h)[..., 3:])
    _optimal(tag + " alpha", dec[..., 3:], pal, src[..., 3:])
    _solid(tag + " alpha", dec, src, [3], [0])
    a = src[..., 3]
    assert np.all(dec[..., 3][a == 255] == 255) and np.all(dec[..., 3][a == 0] == 0), (tag, "fully opaque / transparent texels moved")


def props_etc1(tag, blocks, src, exact):
    """The colour half: exact for an ETC1S source (it is a re-pack); for a UASTC source every texel's modifier is the nearest of its
    half-block's four.  with `etc2`: a differential block's base + delta stays inside 0 .. 31 (else ETC2 reads T / H / planar)."""
    from helpers import etc1_decode_blocks
    h, w = src.shape[:2]
    dec = etc1_decode_blocks(blocks, w, h)
    b = blocks.astype(np.int64)
    diff = (b[..., 3] >> 1) & 1
    for c in range(3):
        d3 = b[..., c] & 7; d3 = np.where(d3 >= 4, d3 - 8, d3); s5 = (b[..., c] >> 3) + d3
        assert np.all((diff == 0) | ((s5 >= 0) & (s5 <= 31))), (tag, "differential base + delta leaves 0 .. 31: an ETC2 decoder reads another mode")
    if exact:
        assert np.array_equal(dec[..., :3], src[..., :3]), (tag, "the ETC1 re-pack is not exact")
        return
    pal = []
    for j in range(4):
        p = blocks.copy(); p[..., 4:6] = 255 * (j >> 1); p[..., 6:8] = 255 * (j & 1)
        pal.append(etc1_decode_blocks(p, w, h)[..., :3])
    _optimal(tag + " modifiers", dec[..., :3], pal, src[..., :3])


def props_eac(tag, blocks, src):
    from helpers import eac_alpha_decode_blocks
    h, w = src.shape[:2]
    dec = eac_alpha_decode_blocks(blocks, w, h)[..., None]
    assert np.all((blocks[..., 1] >> 4) >= 1), (tag, "EAC multiplier 0")
    pal = []
    for j in range(8):
        p = blocks.copy(); bits = sum(j << (3 * i) for i in range(16))
        for k in range(6):
            p[..., 2 + k] = (bits >> (40 - 8 * k)) & 255
        pal.append(eac_alpha_decode_blocks(p, w, h)[..., None])
    _optimal(tag + " alpha", dec, pal, src[..., 3:])
    _solid(tag + " alpha", np.concatenate([np.zeros(dec.shape[:2] + (3,), np.uint8), dec], -1), src, [3], [0])


def check_properties(tag, target, blocks, src, etc1s_source):
    """blocks [by, bx, unit] of `target`, src [h, w, 4] the pinned decoder's texels of the same area."""
    if target == "bc7":
        props_bc7(tag, blocks, src)
    elif target == "bc1":
        props_bc1(tag, blocks, src, False)
    elif target == "bc3":
        props_bc3(tag, blocks, src)
    elif target == "etc1":
        props_etc1(tag, blocks, src, etc1s_source)
    elif target == "etc2_rgba":
        props_eac(tag, blocks[..., :8], src); props_etc1(tag, blocks[..., 8:], src, etc1s_source)
    else:
        raise ValueError(target)


# ------------------------------------------------------------------------------------------------
# one file through every target
# ------------------------------------------------------------------------------------------------
def _count(counters, key, cnt):
    tot = counters.setdefault(key, {})
    for k, v in cnt.items():
        tot[k] = tot.get(k, 0) + int(v)


def _geometry(counters, w, h):
    _count(counters, "geometry", dict(partial_right=int(w % 4 != 0), partial_bottom=int(h % 4 != 0), whole=int(w % 4 == 0 and h % 4 == 0)))


def _strip(px):
    """[n, 16, 4] raster texels of n blocks -> the image [4, 4 n, 4] of those blocks side by side."""
    n = len(px)
    return px.reshape(n, 4, 4, 4).transpose(1, 0, 2, 3).reshape(4, 4 * n, 4)


def check_etc1s_file(oracle, cd, name, data, counters, targets=R.ETC1S_TARGETS, got_all=None):
    """Layers (a) and (b) for one ETC1S file; got_all: target -> blocks already transcoded (a batch call), else one call per target."""
    import uvol
    d = oracle.ktx2_decode(data)
    L = max(1, d.layers); nb = d.bx * d.by
    for l in range(L):
        assert np.array_equal(R.etc1s_rebuild(d, l), d.images[l]), (name, l, "the reference's reading of the tables")
    _geometry(counters, d.width, d.height)
    tup = R.etc1s_tuples(d)

    def describe(l, y, x):
        t = tup[l, y * d.bx + x]
        s = "colour ei %d %s si %d %08x" % (t[0], d.endpoints[t[0]].tolist(), t[1], d.selectors[t[1]])
        return s + (" alpha ei %d %s si %d %08x" % (t[2], d.endpoints[t[2]].tolist(), t[3], d.selectors[t[3]]) if len(t) == 4 else "")
    for target in targets:
        if target == "bc1" and d.has_alpha:
            if got_all is None:
                outs, st = cd.transcode_texture_segments_status([data], "bc1")
                assert st == [uvol.UVOL_E_UNSUPPORTED] and outs[0] is None
            continue
        if got_all is None:
            (got,), st = cd.transcode_texture_segments_status([data], target)
            assert st == [uvol.UVOL_OK], (name, target, st)
        else:
            got = got_all[target]
        want, cnt, inv, first = R.etc1s_reference(d, target)
        _count(counters, ("etc1s", target), cnt)
        assert_blocks_equal(name, target, got, want, describe)
        if L * nb <= WHOLE_LAYER_BLOCKS:
            for l in range(L):
                check_properties("%s -> %s layer %d" % (name, target, l), target, got[l], d.images[l], True)
        else:
            assert d.width % 4 == 0 and d.height % 4 == 0
            src = np.stack(d.images).reshape(L, d.by, 4, d.bx, 4, 4).transpose(0, 1, 3, 2, 4, 5).reshape(L * nb, 16, 4)[first]
            check_properties("%s -> %s distinct tuples" % (name, target), target, got.reshape(L * nb, -1)[first][None], _strip(src), True)
    return d


def sample_mask(L, by, bx, seed, interior=16384):
    """Every block of the border rows / columns plus a seeded sample of `interior` interior blocks per layer."""
    m = np.zeros((L, by, bx), bool); m[:, [0, -1], :] = True; m[:, :, [0, -1]] = True
    rng = np.random.default_rng(seed)
    for l in range(L):
        inner = np.argwhere(~m[l]); pick = inner[rng.choice(len(inner), size=min(interior, len(inner)), replace=False)]
        m[l, pick[:, 0], pick[:, 1]] = True
    return m


def check_uastc_file(oracle, cd, name, data, counters, targets=R.UASTC_TARGETS, got_all=None, sampled=()):
    """Layers (a) and (b) for one UASTC file.  Targets named in `sampled` are judged on sample_mask's blocks only (the EAC search of a
    full-size layer of distinct alpha blocks is too slow for the reference); every other target on every block."""
    import uvol
    info = oracle.uastc_ktx2_info(data); blk = R.uastc_file_blocks(data, info)
    L, by, bx = blk.shape[:3]; w, h = info["width"], info["height"]
    _geometry(counters, w, h)
    u, first, inv = np.unique(blk.reshape(-1, 16), axis=0, return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    px = oracle.uastc_decode_blocks(u)
    img = px[inv].reshape(L, by, bx, 4, 4, 4).transpose(0, 1, 3, 2, 4, 5).reshape(L, by * 4, bx * 4, 4)[:, :h, :w]
    assert np.array_equal(img, oracle.uastc_ktx2_decode(data)), (name, "the reference's reading of the container")
    modes = {}
    for i in range(0, len(u), max(1, len(u) // 4000)):                        # (a stride over the distinct blocks: the census needs presence, not totals)
        m = oracle.uastc_unpack(u[i]).mode; modes["mode%d" % m] = modes.get("mode%d" % m, 0) + 1
    _count(counters, ("uastc", "modes"), modes)

    def describe(l, y, x):
        return "UASTC block %s texels %s" % (_hex(blk[l, y, x]), _hex(px[inv[(l * by + y) * bx + x]]))
    for target in targets:
        if got_all is None:
            (got,), st = cd.transcode_texture_segments_status([data], target)
            assert st == [uvol.UVOL_OK], (name, target, st)
        else:
            got = got_all[target]
        if target in sampled:
            mask = sample_mask(L, by, bx, seed=7)
            sel = np.unique(inv[mask.reshape(-1)])
        else:
            mask = None; sel = np.arange(len(u))
        ref_u, cnt = R.uastc_reference(px[sel], target)
        _count(counters, ("uastc", target), cnt)
        full = np.zeros((len(u), ref_u.shape[1]), np.uint8); full[sel] = ref_u
        want = full[inv].reshape(L, by, bx, -1)
        assert_blocks_equal(name, target, got, want, describe, mask)
        check_properties("%s -> %s distinct blocks" % (name, target), target, got.reshape(L * by * bx, -1)[first[sel]][None], _strip(px[sel]), False)


# ------------------------------------------------------------------------------------------------
# the case table
# ------------------------------------------------------------------------------------------------
# Every branch of the documented rules that the case table must reach (the counters come from the reference alone).
REQUIRED = {
    ("etc1s", "bc7"): ("mode5", "mode6", "tie", "swap", "no_swap", "alpha_swap", "alpha_no_swap"),
    ("etc1s", "etc2_rgba"): ("eac_constant", "eac_clamped", "eac_exit0", "eac_searched"),
    ("etc1s", "bc1"): ("bc1_plain", "bc1_equal"),           # bc1_swap: unreachable for ETC1S sources - test_etc1s_bc1_never_swaps
    ("etc1s", "bc3"): ("bc4_equal", "bc4_range", "bc1_plain", "bc1_equal"),
    ("uastc", "etc1"): ("etc1_differential", "etc1_individual", "etc1_flip0", "etc1_flip1") + tuple("etc1_table%d" % t for t in range(8)),
    ("uastc", "etc2_rgba"): ("eac_constant", "eac_clamped", "eac_exit0", "eac_searched", "etc1_differential", "etc1_individual"),
    ("uastc", "bc1"): ("bc1_plain", "bc1_swap", "bc1_equal", "cov_rg_negative", "cov_bg_negative"),
    ("uastc", "bc3"): ("bc4_equal", "bc4_range", "bc1_swap", "bc1_equal"),
    ("uastc", "modes"): tuple("mode%d" % m for m in (0, 6, 8, 10, 11, 12, 18)),
    "geometry": ("partial_right", "partial_bottom", "whole"),
}


def assert_coverage(counters):
    missing = [(k, c) for k, need in REQUIRED.items() for c in need if counters.get(k, {}).get(c, 0) <= 0]
    assert not missing, ("the case table does not reach these branches", missing, counters)


def small_case_files(oracle):
    """name -> (ETC1S file, UASTC file) of the case table, encoded by the pinned encoders of oracle/."""
    return {nm: (oracle.ktx2_encode(TC.case_layers(nm)), oracle.uastc_ktx2_encode(TC.case_layers(nm))) for nm, *_ in TC.SMALL_CASES}


def check_case_table(oracle, cd, counters):
    from conftest import GOLDEN
    for nm, (fe, fu) in small_case_files(oracle).items():
        check_etc1s_file(oracle, cd, nm, fe, counters)
        check_uastc_file(oracle, cd, nm + " (uastc)", fu, counters)
    check_etc1s_file(oracle, cd, "00000.ktx2", open(os.path.join(GOLDEN, "00000.ktx2"), "rb").read(), counters)


def check_mixed_batch(oracle, cd):
    """One uvol_transcode_texture_segments_st call per target over ten files: six of one shape (the ABI takes one shape per call) with
    opaque and alpha ETC1S files alternating and two UASTC files among them, plus two ETC1S files of other sizes and layer counts, which fail in
    their own slots (UVOL_E_INVALID) as the header documents.  Job indexing, per-file output strides, the UNSUPPORTED slots of BC1 / ETC1 for
    alpha files: every accepted file's blocks equal the reference's, whatever stood next to it."""
    import uvol
    same, other = TC.batch_layers()
    files = [oracle.ktx2_encode(s) for s in same]
    uf = [oracle.uastc_ktx2_encode(same[1]), oracle.uastc_ktx2_encode(same[2])]
    odd = [oracle.ktx2_encode(o) for o in other]
    batch = [files[0], files[1], odd[0], uf[0], files[2], files[3], odd[1], files[4], uf[1], files[5]]
    kind = ["o", "a", "x", "u", "o", "a", "x", "o", "u", "a"]
    counters = {}
    for target in ("bc7", "etc2_rgba", "bc1", "bc3", "etc1"):
        outs, st = cd.transcode_texture_segments_status(batch, target)
        for i, (f, k) in enumerate(zip(batch, kind)):
            tag = "batch[%d]" % i
            if k == "x":
                assert st[i] == uvol.UVOL_E_INVALID and outs[i] is None, (target, i, st)
            elif k == "a" and target in ("bc1", "etc1"):
                assert st[i] == uvol.UVOL_E_UNSUPPORTED and outs[i] is None, (target, i, st)
            elif k == "u":
                assert st[i] == uvol.UVOL_OK, (target, i, st)
                if target != "bc7":                                           # (UASTC -> BC7 is pinned by oracle/uastc.c)
                    check_uastc_file(oracle, cd, tag, f, counters, targets=(target,), got_all={target: outs[i]})
                else:
                    assert np.array_equal(outs[i], oracle.uastc_ktx2_decode(f, "bc7")), (target, i)
            else:
                assert st[i] == uvol.UVOL_OK, (target, i, st)
                if target != "etc1":                                          # (ETC1S -> ETC1 is the exact re-pack)
                    check_etc1s_file(oracle, cd, tag, f, counters, targets=(target,), got_all={target: outs[i]})
                else:
                    d = oracle.ktx2_decode(f); tup = R.etc1s_tuples(d)
                    want = R.etc1_repack(d.endpoints[tup[..., 0].reshape(-1)], d.selectors[tup[..., 1].reshape(-1)]).reshape(outs[i].shape)
                    assert np.array_equal(outs[i], want), (target, i)
    # the files of another shape are good files: alone they pass
    for j, f in enumerate(odd):
        check_etc1s_file(oracle, cd, "batch other[%d]" % j, f, counters, targets=("bc7", "bc3"))


# ------------------------------------------------------------------------------------------------
# tests
# ------------------------------------------------------------------------------------------------
def test_hipemu_transcode_case_table_blocks_equal_reference(oracle, hipemu_lib):
    """Every block of every target over the case table (4 x 4, 13 x 7, 37 x 50, 52^2, 256^2 x 5, opaque and with alpha, ETC1S and UASTC, and the
    reference's own 1024^2 x 5 fixture): layers (a) and (b), and the coverage condition - the reference's branch counters show that the
    table reaches every branch of every rule (REQUIRED)."""
    import uvol
    cd = uvol.Codec(lib_path=hipemu_lib)
    counters = {}
    try:
        check_case_table(oracle, cd, counters)
    finally:
        cd.close()
    assert_coverage(counters)


def test_hipemu_transcode_mixed_batch(oracle, hipemu_lib):
    import uvol
    cd = uvol.Codec(lib_path=hipemu_lib)
    try:
        check_mixed_batch(oracle, cd)
    finally:
        cd.close()


def test_etc1s_bc1_never_swaps():
    """The ETC1S -> BC1 branch the case table cannot reach, exempted by enumeration: a block's colour mapping depends on its endpoint and on
    the lowest / highest selector it uses alone - 32^3 x 8 endpoints x 10 selector ranges.  Through the reference, for all 2,621,440: colour0 >=
    colour1 before any swap (the brightest used colour is not below the darkest in any channel), so the endpoint swap of k_tdec_bc13 never runs
    for an ETC1S source (it does for UASTC sources: REQUIRED); endpoints are equal for every one-selector block and for no block that uses the
    full range 0 .. 3 (its colours differ by 8 or more in some channel even when clamped, more than one RGB565 step)."""
    g = np.arange(32)
    e = np.stack(np.meshgrid(g, g, g, np.arange(8), indexing="ij"), -1).reshape(-1, 4)
    assert len(e) == 262144
    for klo in range(4):
        for khi in range(klo, 4):
            sel = np.full(len(e), klo | sum(khi << (2 * i) for i in range(1, 16)), np.int64)            # texel 0 on klo, the others on khi
            swap = equal = 0
            for s0 in range(0, len(e), 65536):
                _, cnt = R.ref_etc1s_bc1(e[s0:s0 + 65536], sel[s0:s0 + 65536]); swap += cnt["bc1_swap"]; equal += cnt["bc1_equal"]
            assert swap == 0, (klo, khi, swap)
            assert equal == len(e) if klo == khi else True, (klo, khi, equal)
            assert equal == 0 if (klo, khi) == (0, 3) else True, (klo, khi, equal)


def test_vectorised_bc1_bc3_helpers_equal_the_block_at_a_time_decoders():
    """tests/helpers.py decodes BC1 / BC3 all blocks at once since the block-by-block checks need it on whole segments; the original
    block-at-a-time decoders stay beside them and both give the same texels on random blocks (three- and four-colour BC1, both BC4 modes)."""
    from helpers import bc1_decode_blocks, bc1_decode_blocks_scalar, bc3_decode_blocks, bc3_decode_blocks_scalar
    rng = np.random.default_rng(5)
    b = rng.integers(0, 256, (7, 11, 16)).astype(np.uint8)
    b[0, 0, 10:12] = b[0, 0, 8:10]; b[0, 1, 0] = b[0, 1, 1]
    for w, h in ((44, 28), (41, 26)):
        assert np.array_equal(bc1_decode_blocks(b[..., 8:], w, h), bc1_decode_blocks_scalar(b[..., 8:], w, h))
        assert np.array_equal(bc1_decode_blocks(b[..., 8:], w, h, True), bc1_decode_blocks_scalar(b[..., 8:], w, h, True))
        assert np.array_equal(bc3_decode_blocks(b, w, h), bc3_decode_blocks_scalar(b, w, h))
