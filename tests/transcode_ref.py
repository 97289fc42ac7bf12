"""Plain NumPy references of the re-fit transcode targets (test infrastructure only: the product never imports this module).

One function per target, written from the rules in the comments above the kernels (csrc/tex_decode.hip K3'b / K3'c / K3'',
csrc/tex_uastc.hip targets 3 - 6) and from the public block formats.  Integer arithmetic in int64, vectorised over blocks.  Inputs come
from the fixture-pinned decoders of oracle/: `oracle.ktx2_decode` (ETC1S: endpoints, selectors, block_ei, block_si) and
`oracle.uastc_decode_blocks` (UASTC: all 16 texels of a block, the padding texels of ragged images included).  A block's result depends
only on its source tuple, so every function works on the DISTINCT tuples of a file and the drivers scatter the results: whole segments are
checked, not samples.  Every function returns its blocks and a dict of branch counters (how often each branch of the rule was taken).

Texel order everywhere: raster, i = 4 * y + x.  An ETC1S selector word holds texel (x, y) at bits 8 * y + 2 * x = 2 * i."""
import numpy as np

INTEN = np.array([[-8, -2, 2, 8], [-17, -5, 5, 17], [-29, -9, 9, 29], [-42, -13, 13, 42], [-60, -18, 18, 60], [-80, -24, 24, 80],
                  [-106, -33, 33, 106], [-183, -47, 47, 183]], np.int64)
ETC1_MAG = np.array([[2, 8], [5, 17], [9, 29], [13, 42], [18, 60], [24, 80], [33, 106], [47, 183]], np.int64)
ETC1_MOD = np.stack([ETC1_MAG[:, 0], ETC1_MAG[:, 1], -ETC1_MAG[:, 0], -ETC1_MAG[:, 1]], 1)          # [table, ETC1 pixel index]
EAC_MOD = np.array([[-3, -6, -9, -15, 2, 5, 8, 14], [-3, -7, -10, -13, 2, 6, 9, 12], [-2, -5, -8, -13, 1, 4, 7, 12], [-2, -4, -6, -13, 1, 3, 5, 12],
                    [-3, -6, -8, -12, 2, 5, 7, 11], [-3, -7, -9, -11, 2, 6, 8, 10], [-4, -7, -8, -11, 3, 6, 7, 10], [-3, -5, -8, -11, 2, 4, 7, 10],
                    [-2, -6, -8, -10, 1, 5, 7, 9], [-2, -5, -8, -10, 1, 4, 7, 9], [-2, -4, -8, -10, 1, 3, 7, 9], [-2, -5, -7, -10, 1, 4, 6, 9],
                    [-3, -4, -7, -10, 2, 3, 6, 9], [-1, -2, -3, -10, 0, 1, 2, 9], [-4, -6, -8, -9, 3, 5, 7, 8], [-3, -5, -7, -9, 2, 4, 6, 8]], np.int64)
BC7_W2 = np.array([0, 21, 43, 64], np.int64)
BC7_W4 = np.array([0, 4, 9, 13, 17, 21, 26, 30, 34, 38, 43, 47, 51, 55, 60, 64], np.int64)
ETC1S_TARGETS = ("bc7", "etc2_rgba", "bc1", "bc3")
UASTC_TARGETS = ("etc1", "etc2_rgba", "bc1", "bc3")


class _Bits:
    """n blocks of nbits bits, filled field by field, least significant bit first; bytes() packs them little-endian."""
    def __init__(self, n, nbits):
        self.b = np.zeros((n, nbits), np.uint8); self.pos = 0

    def put(self, v, nb):
        v = np.broadcast_to(np.asarray(v, np.int64), (self.b.shape[0],))
        assert np.all((v >= 0) & (v < (1 << nb)))
        for k in range(nb):
            self.b[:, self.pos + k] = (v >> k) & 1
        self.pos += nb

    def bytes(self):
        assert self.pos == self.b.shape[1]
        return np.packbits(self.b, axis=1, bitorder="little")


def _sel(sel):
    """Selector words [n] -> the 16 two-bit selectors [n, 16] in raster order."""
    return (np.asarray(sel, np.int64)[:, None] >> (2 * np.arange(16))) & 3


def _first_argmin(d):
    """Index of the first smallest entry along the last axis (np.argmin's documented rule) and that entry."""
    j = d.argmin(-1)
    return j, np.take_along_axis(d, j[..., None], -1)[..., 0]


# ------------------------------------------------------------------------------------------------
# ETC1S sources
# ------------------------------------------------------------------------------------------------
def etc1s_colours(e):
    """Endpoints [n, 4] (R5, G5, B5, intensity table) -> the block's four colours [n, 4, 3], dark to bright, clamped per channel."""
    e = np.asarray(e, np.int64)
    base = (e[:, :3] << 3) | (e[:, :3] >> 2)
    return np.clip(base[:, None, :] + INTEN[e[:, 3] & 7][:, :, None], 0, 255)


def etc1s_levels(e):
    """The four levels of an alpha-slice block: the green endpoint widened, plus the intensity table, clamped.  [n, 4]"""
    e = np.asarray(e, np.int64)
    g = (e[:, 1] << 3) | (e[:, 1] >> 2)
    return np.clip(g[:, None] + INTEN[e[:, 3] & 7], 0, 255)


def etc1s_rebuild(d, layer):
    """The RGBA image of a layer rebuilt from the decoded tables alone (5-bit base widened, intensity table, clamp, selector of texel
    (x, y) at bits 8 y + 2 x; alpha from slice 2 l + 1, green endpoint).  Equality with the pinned decoder's image proves this module's
    reading of the tables before anything is judged with it."""
    ash = 1 if d.has_alpha else 0
    sl = layer << ash
    col = etc1s_colours(d.endpoints[d.block_ei[sl]]); s = _sel(d.selectors[d.block_si[sl]])
    nb = col.shape[0]
    px = np.full((nb, 16, 4), 255, np.int64)
    px[..., :3] = col[np.arange(nb)[:, None], s]
    if ash:
        lv = etc1s_levels(d.endpoints[d.block_ei[sl + 1]]); sa = _sel(d.selectors[d.block_si[sl + 1]])
        px[..., 3] = lv[np.arange(nb)[:, None], sa]
    img = px.reshape(d.by, d.bx, 4, 4, 4).transpose(0, 2, 1, 3, 4).reshape(d.by * 4, d.bx * 4, 4)
    return img[:d.height, :d.width].astype(np.uint8)


def _used_ends(values, s):
    """values [n, 4, ...] (dark to bright), s [n, 16] selectors -> the entries of the lowest / highest selector the block uses."""
    ar = np.arange(len(values))
    return values[ar, s.min(1)], values[ar, s.max(1)]


def ref_etc1s_bc7(e, sel, ae=None, asel=None):
    """K3'': ETC1S block (endpoint, selector word; with ae / asel the block of the alpha slice) -> BC7 mode 5 or 6, [n, 16] uint8."""
    n = len(e); col = etc1s_colours(e); s = _sel(sel)
    lo, hi = _used_ends(col, s); lo7 = lo >> 1; hi7 = hi >> 1
    hist = np.stack([(s == k).sum(1) for k in range(4)], 1)
    l5 = (lo7 << 1) | (lo7 >> 6); h5 = (hi7 << 1) | (hi7 >> 6)
    p5 = (l5[:, None, :] * (64 - BC7_W2)[None, :, None] + h5[:, None, :] * BC7_W2[None, :, None] + 32) >> 6              # [n, w, c]
    p6 = ((2 * lo7 + 1)[:, None, :] * (64 - BC7_W4)[None, :, None] + (2 * hi7 + 1)[:, None, :] * BC7_W4[None, :, None] + 32) >> 6
    idx5, e5 = _first_argmin(((p5[:, None] - col[:, :, None]) ** 2).sum(-1))                                               # [n, k]
    idx6, e6 = _first_argmin(((p6[:, None] - col[:, :, None]) ** 2).sum(-1))
    err5 = (hist * e5).sum(1); err6 = (hist * e6).sum(1)
    alpha = ae is not None
    use5 = (err5 <= err6) | alpha
    if alpha:
        al = etc1s_levels(ae); sa = _sel(asel); a_lo, a_hi = _used_ends(al, sa)
        pa = (a_lo[:, None] * (64 - BC7_W2) + a_hi[:, None] * BC7_W2 + 32) >> 6
        aidx, _ = _first_argmin((pa[:, None, :] - al[:, :, None]) ** 2)
    else:
        sa = np.zeros((n, 16), np.int64); a_lo = a_hi = np.full(n, 255, np.int64); aidx = np.zeros((n, 4), np.int64)
    ar = np.arange(n)[:, None]
    # mode 5
    i5 = idx5[ar, s]; swap5 = i5[:, 0] >= 2
    ia = aidx[ar, sa]; aswap = ia[:, 0] >= 2
    b5 = _Bits(n, 128); b5.put(1 << 5, 6); b5.put(0, 2)
    for c in range(3):
        b5.put(np.where(swap5, hi7[:, c], lo7[:, c]), 7); b5.put(np.where(swap5, lo7[:, c], hi7[:, c]), 7)
    b5.put(np.where(aswap, a_hi, a_lo), 8); b5.put(np.where(aswap, a_lo, a_hi), 8)
    for i in range(16):
        b5.put(np.where(swap5, 3 - i5[:, i], i5[:, i]), 1 if i == 0 else 2)
    for i in range(16):
        b5.put(np.where(aswap, 3 - ia[:, i], ia[:, i]), 1 if i == 0 else 2)
    # mode 6
    i6 = idx6[ar, s]; swap6 = i6[:, 0] >= 8
    b6 = _Bits(n, 128); b6.put(1 << 6, 7)
    for c in range(3):
        b6.put(np.where(swap6, hi7[:, c], lo7[:, c]), 7); b6.put(np.where(swap6, lo7[:, c], hi7[:, c]), 7)
    b6.put(127, 7); b6.put(127, 7); b6.put(1, 1); b6.put(1, 1)
    for i in range(16):
        b6.put(np.where(swap6, 15 - i6[:, i], i6[:, i]), 3 if i == 0 else 4)
    out = np.where(use5[:, None], b5.bytes(), b6.bytes())
    swap = np.where(use5, swap5, swap6)
    cnt = dict(mode5=int(use5.sum()), mode6=int((~use5).sum()), tie=int((err5 == err6).sum()) if not alpha else 0,
               swap=int(swap.sum()), no_swap=int((~swap).sum()))
    if alpha:
        cnt.update(alpha_swap=int(aswap.sum()), alpha_no_swap=int((~aswap).sum()))
    return out, cnt


_EAC_E = None


def _eac_table():
    """E[t, m - 1, base, a] = the squared distance of alpha a from the nearest of the eight levels clamp(base + m * EAC_MOD[t][j])."""
    global _EAC_E
    if _EAC_E is None:
        E = np.zeros((16, 15, 256, 256), np.uint16); a = np.arange(256)
        for t in range(16):
            for m in range(1, 16):
                lv = np.clip(np.arange(256)[:, None] + m * EAC_MOD[t][None, :], 0, 255)                      # [base, j]
                E[t, m - 1] = ((lv[:, :, None] - a[None, None, :]) ** 2).min(1)
        _EAC_E = E
    return _EAC_E


def _eac_counters(levels, weights, bb, bm, bt, shortcut):
    """Branch counters of the EAC search: constant alpha, a winner with levels that clamp, a winner of error 0 (the search's early exit)."""
    used = weights > 0
    const = np.where(used, levels, 255).min(1) == np.where(used, levels, 0).max(1)
    raw = bb[:, None] + bm[:, None] * EAC_MOD[bt]; lv = np.clip(raw, 0, 255)
    err = (((lv[:, None, :] - levels[:, :, None]) ** 2).min(-1) * weights).sum(1)
    searched = ~(const & shortcut)
    return dict(eac_constant=int(const.sum()), eac_clamped=int(((raw < 0) | (raw > 255)).any(1).sum()), eac_exit0=int(((err == 0) & searched).sum()),
                eac_searched=int(searched.sum()))


def eac_fit(levels, weights, shortcut, dedupe=True):
    """The EAC alpha search both kernels share.  levels [n, K]: the alpha values to fit, weights [n, K]: how many texels carry each
    (0: unused).  mid = (lowest + highest used level + 1) >> 1; every (table 0..15, multiplier 1..15, base mid - 2 .. mid + 2 inside
    0..255) in that order, error = sum of weight * squared distance to the nearest of the eight clamped EAC levels; the first best wins.
    shortcut (UASTC path): lowest == highest takes table 13, multiplier 1, base = that value without a search.
    -> base, multiplier, table [n], the index of the nearest EAC level (first best) for every entry of levels [n, K], counters."""
    levels = np.asarray(levels, np.int64); weights = np.asarray(weights, np.int64)
    if dedupe:                                             # the search is a function of (levels, weights): once per distinct row
        u, inv = np.unique(np.concatenate([levels, weights], 1), axis=0, return_inverse=True); inv = inv.reshape(-1)
        bb, bm, bt, lj, _ = eac_fit(u[:, :levels.shape[1]], u[:, levels.shape[1]:], shortcut, dedupe=False)
        bb, bm, bt, lj = bb[inv], bm[inv], bt[inv], lj[inv]
        return bb, bm, bt, lj, _eac_counters(levels, weights, bb, bm, bt, shortcut)
    n, K = levels.shape; E = _eac_table()
    used = weights > 0
    lo = np.where(used, levels, 255).min(1); hi = np.where(used, levels, 0).max(1)
    mid = (lo + hi + 1) >> 1
    bt = np.zeros(n, np.int64); bm = np.ones(n, np.int64); bb = mid.copy(); best = np.zeros(n, np.int64)
    T = np.arange(16)[:, None, None, None, None]; M = np.arange(15)[None, :, None, None, None]
    step = 96
    for s0 in range(0, n, step):
        sl = slice(s0, min(n, s0 + step))
        base = mid[sl, None] + np.arange(-2, 3)[None, :]; ok = (base >= 0) & (base <= 255)
        g = E[T, M, np.clip(base, 0, 255)[None, None, :, :, None], levels[sl][None, None, :, None, :]].astype(np.int64)      # [t, m, c, db, K]
        err = (g * weights[sl][None, None, :, None, :]).sum(-1).transpose(2, 0, 1, 3)                                           # [c, t, m, db]
        err = np.where(ok[:, None, None, :], err, 1 << 40).reshape(err.shape[0], -1)
        j, b = _first_argmin(err)
        bt[sl] = j // 75; bm[sl] = (j // 5) % 15 + 1; bb[sl] = mid[sl] + (j % 5) - 2; best[sl] = b
    const = lo == hi
    if shortcut:
        bt = np.where(const, 13, bt); bm = np.where(const, 1, bm); bb = np.where(const, hi, bb); best = np.where(const, 0, best)
    raw = bb[:, None] + bm[:, None] * EAC_MOD[bt]                                                                               # [n, j]
    lv = np.clip(raw, 0, 255)
    lj, _ = _first_argmin((lv[:, None, :] - levels[:, :, None]) ** 2)
    cnt = None
    return bb, bm, bt, lj, cnt


def eac_pack(base, mult, tab, idx):
    """EAC alpha block: base, multiplier << 4 | table, then 16 x 3-bit indices, pixel 4 x + y first, in the top bits.  idx [n, 16] raster."""
    n = len(base); bits = np.zeros(n, np.int64)
    for y in range(4):
        for x in range(4):
            bits |= idx[:, 4 * y + x] << (45 - 3 * (4 * x + y))
    return np.stack([base, (mult << 4) | tab] + [(bits >> (40 - 8 * k)) & 255 for k in range(6)], 1).astype(np.uint8)


def etc1_repack(e, sel):
    """K3': an ETC1S block as the ETC1 differential block it is (zero delta, one table for both halves); selector 0..3 -> ETC1 index 3, 2, 0, 1."""
    e = np.asarray(e, np.int64); s = _sel(sel); idx = np.array([3, 2, 0, 1], np.int64)[s]
    msb = np.zeros(len(e), np.int64); lsb = np.zeros(len(e), np.int64)
    for y in range(4):
        for x in range(4):
            msb |= (idx[:, 4 * y + x] >> 1) << (4 * x + y); lsb |= (idx[:, 4 * y + x] & 1) << (4 * x + y)
    t = e[:, 3] & 7
    return np.stack([e[:, 0] << 3, e[:, 1] << 3, e[:, 2] << 3, (t << 5) | (t << 2) | 2, msb >> 8, msb & 255, lsb >> 8, lsb & 255], 1).astype(np.uint8)


def ref_etc1s_etc2a(e, sel, ae=None, asel=None):
    """K3'b: EAC alpha block of the alpha slice's four levels (an opaque file: sixteen texels of 255), then the ETC1 re-pack.  [n, 16]"""
    n = len(e)
    if ae is not None:
        al = etc1s_levels(ae); sa = _sel(asel); w = np.stack([(sa == k).sum(1) for k in range(4)], 1)
    else:
        al = np.full((n, 4), 255, np.int64); sa = np.zeros((n, 16), np.int64); w = np.tile(np.array([16, 0, 0, 0], np.int64), (n, 1))
    bb, bm, bt, lj, cnt = eac_fit(al, w, shortcut=False)
    a = eac_pack(bb, bm, bt, lj[np.arange(n)[:, None], sa])
    return np.concatenate([a, etc1_repack(e, sel)], 1), cnt


def bc4_fit(levels, used, idx):
    """BC4 alpha block: alpha0 = the highest, alpha1 = the lowest used level; eight-value mode (value j = alpha0, alpha1, then
    ((8 - j) alpha0 + (j - 1) alpha1) / 7); every level takes the first nearest value; equal endpoints: index 0 everywhere.
    levels [n, K], used [n, K] bool, idx [n, 16]: which level each texel carries.  -> [n, 8] uint8, counters."""
    levels = np.asarray(levels, np.int64); n = len(levels)
    a0 = np.where(used, levels, 0).max(1); a1 = np.where(used, levels, 255).min(1)
    j = np.arange(8)
    pal = np.where(j == 0, a0[:, None], np.where(j == 1, a1[:, None], ((8 - j) * a0[:, None] + (j - 1) * a1[:, None]) // 7))
    lj, _ = _first_argmin((pal[:, None, :] - levels[:, :, None]) ** 2)
    lj = np.where((a0 > a1)[:, None], lj, 0)
    tx = lj[np.arange(n)[:, None], idx]
    bits = np.zeros(n, np.int64)
    for i in range(16):
        bits |= tx[:, i] << (3 * i)
    out = np.stack([a0, a1] + [(bits >> (8 * k)) & 255 for k in range(6)], 1).astype(np.uint8)
    return out, dict(bc4_equal=int((a0 == a1).sum()), bc4_range=int((a0 > a1).sum()))


def bc1_fit(hi, lo, colours, idx):
    """BC1 colour block.  hi / lo [n, 3]: the 8-bit colours that become colour0 / colour1 (rounded to 5 / 6 / 5 bits: (v * 31 + 127) / 255,
    (v * 63 + 127) / 255); palette c0, c1, (2 c0 + c1) / 3, (c0 + 2 c1) / 3 of the widened endpoints; each of colours [n, K, 3] takes the
    first nearest entry (squared error over R, G, B); colour0 == colour1: index 0 everywhere; colour0 < colour1: endpoints swapped, indices
    0 <-> 1 and 2 <-> 3.  idx [n, 16]: which colour each texel carries.  -> [n, 8] uint8, counters."""
    n = len(hi); mul = np.array([31, 63, 31], np.int64)
    q0 = (hi * mul + 127) // 255; q1 = (lo * mul + 127) // 255
    c0 = (q0[:, 0] << 11) | (q0[:, 1] << 5) | q0[:, 2]; c1 = (q1[:, 0] << 11) | (q1[:, 1] << 5) | q1[:, 2]

    def widen(q):
        return np.stack([(q[:, 0] << 3) | (q[:, 0] >> 2), (q[:, 1] << 2) | (q[:, 1] >> 4), (q[:, 2] << 3) | (q[:, 2] >> 2)], 1)
    e0, e1 = widen(q0), widen(q1)
    pal = np.stack([e0, e1, (2 * e0 + e1) // 3, (e0 + 2 * e1) // 3], 1)
    mp, _ = _first_argmin(((pal[:, None, :, :] - colours[:, :, None, :]) ** 2).sum(-1))
    mp = np.where((c0 != c1)[:, None], mp, 0)
    sw = c0 < c1
    mp = np.where(sw[:, None], mp ^ 1, mp); c0, c1 = np.where(sw, c1, c0), np.where(sw, c0, c1)
    tx = mp[np.arange(n)[:, None], idx]
    bits = np.zeros(n, np.int64)
    for i in range(16):
        bits |= tx[:, i] << (2 * i)
    out = np.stack([c0 & 255, c0 >> 8, c1 & 255, c1 >> 8] + [(bits >> (8 * k)) & 255 for k in range(4)], 1).astype(np.uint8)
    return out, dict(bc1_swap=int(sw.sum()), bc1_equal=int((c0 == c1).sum()), bc1_plain=int((~sw & (c0 != c1)).sum()))


def ref_etc1s_bc1(e, sel):
    """K3'c, colour: brightest ETC1S colour the block uses -> colour0, darkest -> colour1."""
    col = etc1s_colours(e); s = _sel(sel)
    lo, hi = _used_ends(col, s)
    return bc1_fit(hi, lo, col, s)


def ref_etc1s_bc3(e, sel, ae=None, asel=None):
    """K3'c: BC4 block of the alpha slice's levels (those the block uses give the endpoints; an opaque file: 255, 255, indices 0), then BC1."""
    n = len(e)
    if ae is not None:
        al = etc1s_levels(ae); sa = _sel(asel); used = np.stack([(sa == k).any(1) for k in range(4)], 1)
    else:
        al = np.full((n, 4), 255, np.int64); sa = np.zeros((n, 16), np.int64); used = np.tile(np.array([True, False, False, False]), (n, 1))
    a, ca = bc4_fit(al, used, sa)
    c, cc = ref_etc1s_bc1(e, sel)
    return np.concatenate([a, c], 1), dict(ca, **cc)


# ------------------------------------------------------------------------------------------------
# UASTC sources: px [n, 16, 4] = the decoded texels of a block, raster order
# ------------------------------------------------------------------------------------------------
_RASTER = np.arange(16)[None, :]


def ref_px_bc1(px):
    """Target 3, colour: range fit.  Corners of the bounding box; the R (B) ends swapped where sum((16 r - sum r) >> 4) * ((16 g - sum g) >> 4)
    is negative; each end pulled in by (hi - lo) / 16 (C division: towards zero); then the BC1 block of those two colours."""
    v = np.asarray(px, np.int64)[..., :3]
    mn = v.min(1); mx = v.max(1); sm = v.sum(1)
    r = (16 * v - sm[:, None, :]) >> 4
    cov_rg = (r[..., 0] * r[..., 1]).sum(1); cov_bg = (r[..., 2] * r[..., 1]).sum(1)
    hi = mx.copy(); lo = mn.copy()
    hi[:, 0] = np.where(cov_rg < 0, mn[:, 0], mx[:, 0]); lo[:, 0] = np.where(cov_rg < 0, mx[:, 0], mn[:, 0])
    hi[:, 2] = np.where(cov_bg < 0, mn[:, 2], mx[:, 2]); lo[:, 2] = np.where(cov_bg < 0, mx[:, 2], mn[:, 2])
    d = hi - lo; ins = np.sign(d) * (np.abs(d) // 16)
    out, cnt = bc1_fit(hi - ins, lo + ins, v, np.broadcast_to(_RASTER, (len(v), 16)))
    cnt.update(cov_rg_negative=int((cov_rg < 0).sum()), cov_bg_negative=int((cov_bg < 0).sum()))
    return out, cnt


def ref_px_bc3(px):
    """Target 4: BC4 block of the sixteen alphas (alpha0 the largest, alpha1 the smallest), then the BC1 block."""
    a = np.asarray(px, np.int64)[..., 3]
    ab, ca = bc4_fit(a, np.ones(a.shape, bool), np.broadcast_to(_RASTER, a.shape))
    c, cc = ref_px_bc1(px)
    return np.concatenate([ab, c], 1), dict(ca, **cc)


def ref_px_etc1(px):
    """Target 5: the plain ETC1 fit.  For flip 0 (left | right) and flip 1 (top | bottom): a half's base is its mean colour (sum + 4) >> 3
    rounded to 5 bits ((m * 31 + 127) / 255) when all three deltas second - first fit -4 .. 3 (differential), else to 4 bits ((m * 15 + 127)
    / 255, individual); per half the first table 0 .. 7 with the smallest error when every texel takes its first nearest modifier (pixel
    index order 0 .. 3 = +small, +large, -small, -large); the flip with the smaller total error, flip 0 on a tie."""
    v = np.asarray(px, np.int64)[..., :3]; n = len(v)
    best = None
    for flip in (0, 1):
        half = np.array([(i // 4 >= 2) if flip else (i % 4 >= 2) for i in range(16)], np.int64)
        sm = np.stack([v[:, half == h].sum(1) for h in (0, 1)], 1)                                  # [n, h, c]
        m8 = (sm + 4) >> 3; q5 = (m8 * 31 + 127) // 255; q4 = (m8 * 15 + 127) // 255
        dl = q5[:, 1] - q5[:, 0]; diff = ((dl >= -4) & (dl <= 3)).all(1)
        base = np.where(diff[:, None, None], (q5 << 3) | (q5 >> 2), q4 * 17)
        e = np.zeros((n, 2, 8), np.int64); bis = np.zeros((n, 16, 8), np.int64)
        for i in range(16):
            lv = np.clip(base[:, half[i], None, None, :] + ETC1_MOD[None, :, :, None], 0, 255)        # [n, t, idx, c]
            bi, be = _first_argmin(((lv - v[:, i, None, None, :]) ** 2).sum(-1))                     # [n, t]
            e[:, half[i]] += be; bis[:, i] = bi
        tab, eh = _first_argmin(e)                                                                   # [n, h]
        err = eh.sum(1)
        msb = np.zeros(n, np.int64); lsb = np.zeros(n, np.int64); ar = np.arange(n)
        for y in range(4):
            for x in range(4):
                i = 4 * y + x; bi = bis[ar, i, tab[:, half[i]]]
                msb |= (bi >> 1) << (4 * x + y); lsb |= (bi & 1) << (4 * x + y)
        cb = np.where(diff[:, None], (q5[:, 0] << 3) | (dl & 7), (q4[:, 0] << 4) | q4[:, 1])
        blk = np.concatenate([cb, ((tab[:, 0] << 5) | (tab[:, 1] << 2) | np.where(diff, 2, 0) | flip)[:, None],
                              np.stack([msb >> 8, msb & 255, lsb >> 8, lsb & 255], 1)], 1)
        if best is None:
            best = (err, blk, diff, tab, np.zeros(n, bool))
        else:
            take = err < best[0]
            best = (np.where(take, err, best[0]), np.where(take[:, None], blk, best[1]), np.where(take, diff, best[2]),
                    np.where(take[:, None], tab, best[3]), take)
    err, blk, diff, tab, flipped = best
    cnt = dict(etc1_differential=int(diff.sum()), etc1_individual=int((~diff).sum()), etc1_flip0=int((~flipped).sum()), etc1_flip1=int(flipped.sum()))
    for t in range(8):
        cnt["etc1_table%d" % t] = int((tab == t).any(1).sum())
    return blk.astype(np.uint8), cnt


def ref_px_etc2a(px):
    """Target 6: EAC alpha block of the sixteen alphas (constant alpha: table 13, multiplier 1, base = the value), then the ETC1 fit."""
    a = np.asarray(px, np.int64)[..., 3]
    bb, bm, bt, lj, ca = eac_fit(a, np.ones(a.shape, np.int64), shortcut=True)
    c, cc = ref_px_etc1(px)
    return np.concatenate([eac_pack(bb, bm, bt, lj), c], 1), dict(ca, **cc)


# ------------------------------------------------------------------------------------------------
# drivers: distinct source tuples, scatter
# ------------------------------------------------------------------------------------------------
def _add(total, cnt, weight=None):
    for k, v in cnt.items():
        total[k] = total.get(k, 0) + v


def etc1s_tuples(d):
    """[layers, blocks, 2 or 4]: (endpoint index, selector index) of the colour slice and, for a file with alpha slices, of the alpha slice."""
    L = max(1, d.layers)
    ei = d.block_ei.astype(np.int64); si = d.block_si.astype(np.int64)
    if d.has_alpha:
        return np.stack([ei[0::2], si[0::2], ei[1::2], si[1::2]], -1)[:L]
    return np.stack([ei, si], -1)[:L]


def etc1s_reference(d, target):
    """oracle.ktx2_decode result -> (blocks [layers, by, bx, 8 or 16] uint8 of the target, counters over the file's DISTINCT source tuples,
    inverse: [layers, blocks] index of every block's tuple, first: flat block index of every tuple's first occurrence)."""
    tup = etc1s_tuples(d); L, nb, k = tup.shape
    u, first, inv = np.unique(tup.reshape(-1, k), axis=0, return_index=True, return_inverse=True)
    e = d.endpoints[u[:, 0]]; s = d.selectors[u[:, 1]]
    ae, asel = (d.endpoints[u[:, 2]], d.selectors[u[:, 3]]) if k == 4 else (None, None)
    if target == "bc7":
        out, cnt = ref_etc1s_bc7(e, s, ae, asel)
    elif target == "etc2_rgba":
        out, cnt = ref_etc1s_etc2a(e, s, ae, asel)
    elif target == "bc3":
        out, cnt = ref_etc1s_bc3(e, s, ae, asel)
    elif target == "bc1":
        assert k == 2, "BC1 takes opaque ETC1S files only"
        out, cnt = ref_etc1s_bc1(e, s)
    else:
        raise ValueError(target)
    inv = inv.reshape(L, nb)
    return out[inv].reshape(L, d.by, d.bx, out.shape[1]), cnt, inv, first


def uastc_file_blocks(data, info):
    """The UASTC blocks of a scheme-0 .ktx2 as the container stores them: [layers, by, bx, 16] uint8 from the level's offset."""
    by, bx = (info["height"] + 3) // 4, (info["width"] + 3) // 4; L = info["layers"]
    return np.frombuffer(data, np.uint8, L * by * bx * 16, info["level_off"]).reshape(L, by, bx, 16)


def uastc_reference(px, target, chunk=8192):
    """Decoded texels of distinct UASTC blocks [n, 16, 4] -> (target blocks [n, 8 or 16] uint8, counters)."""
    fn = {"etc1": ref_px_etc1, "etc2_rgba": ref_px_etc2a, "bc1": ref_px_bc1, "bc3": ref_px_bc3}[target]
    outs = []; total = {}
    for s0 in range(0, len(px), chunk):
        o, c = fn(px[s0:s0 + chunk]); outs.append(o); _add(total, c)
    return np.concatenate(outs, 0), total
