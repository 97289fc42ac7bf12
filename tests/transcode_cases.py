"""Input builders for the block-by-block checks of the re-fit transcode targets (tests/test_hipemu_transcode_ref.py,
tests/test_gpu_transcode_ref.py).  Data only: RGBA8 layers [h, w, 4], top row first, made of 16 x 16 tiles that each hold one kind of
content chosen for a place where the kernels branch.  Everything is seeded; nothing is read from disk."""
import numpy as np

TILE = 16


def _blockwise(rng, h, w, lo=0, hi=256):
    """One random colour per 4 x 4 block, [h, w, 3]."""
    c = rng.integers(lo, hi, ((h + 3) // 4, (w + 3) // 4, 3))
    return np.repeat(np.repeat(c, 4, 0), 4, 1)[:h, :w]


def _solid(rng, h, w):
    return _blockwise(rng, h, w)


def _two_colours(rng, h, w):
    a, b = _blockwise(rng, h, w), _blockwise(rng, h, w)
    return np.where(rng.integers(0, 2, (h, w, 1)) == 1, a, b)


def _gradient(rng, h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    s = rng.integers(1, 9, 3); o = rng.integers(0, 120, 3)
    return np.stack([o[0] + s[0] * xx, o[1] + s[1] * yy, o[2] + s[2] * (xx + yy) // 2], -1) % 256


def _noise(rng, h, w):
    return rng.integers(0, 256, (h, w, 3))


def _saturated(rng, h, w):
    """Bases near 0 and 255 with the widest intensity tables: clamping bends the line, the four colours are not collinear."""
    return rng.choice(np.array([0, 255, 3, 250, 128]), size=(h, w, 3), p=[0.3, 0.3, 0.15, 0.15, 0.1])


def _halves(rng, h, w, vertical, close):
    """Half-blocks of unrelated colours (ETC1 individual mode) or of close ones (differential), split left | right or top | bottom."""
    a = _blockwise(rng, h, w, 20, 236)
    b = np.clip(a + rng.integers(-14, 15, a.shape), 0, 255) if close else _blockwise(rng, h, w)
    yy, xx = np.mgrid[0:h, 0:w]
    second = ((xx % 4) >= 2) if vertical else ((yy % 4) >= 2)
    return np.clip(np.where(second[..., None], b, a) + rng.integers(-3, 4, (h, w, 3)), 0, 255)


def _against_green(rng, h, w, channel):
    """R (channel 0) or B (channel 2) running against G inside every block: negative covariance in the UASTC -> BC1 range fit."""
    yy, xx = np.mgrid[0:h, 0:w]
    t = ((xx % 4) + 4 * (yy % 4)) * rng.integers(4, 14) + rng.integers(0, 6, (h, w))
    img = np.stack([t, t, t], -1) + rng.integers(0, 40)
    img[..., channel] = 250 - t
    return np.clip(img, 0, 255)


def _tiny_range(rng, h, w):
    """Ranges below one RGB565 step: BC1 endpoints come out equal."""
    return np.clip(_blockwise(rng, h, w) + rng.integers(0, 3, (h, w, 3)), 0, 255)


def _dark_or_bright(rng, h, w):
    base = _blockwise(rng, h, w, 0, 2) * 255
    return np.clip(base + rng.integers(-90, 91, (h, w, 1)) + rng.integers(-6, 7, (h, w, 3)), 0, 255)


def _smooth(rng, h, w):
    """Low-contrast content: small intensity tables, BC7 mode 6 territory."""
    return np.clip(_blockwise(rng, h, w, 30, 226) + rng.integers(-12, 13, (h, w, 1)) + rng.integers(-2, 3, (h, w, 3)), 0, 255)


COLOUR_KINDS = (
    _solid, _two_colours, _gradient, _noise, _saturated,
    lambda r, h, w: _halves(r, h, w, True, False), lambda r, h, w: _halves(r, h, w, False, False),
    lambda r, h, w: _halves(r, h, w, True, True), lambda r, h, w: _halves(r, h, w, False, True),
    lambda r, h, w: _against_green(r, h, w, 0), lambda r, h, w: _against_green(r, h, w, 2),
    _tiny_range, _dark_or_bright, _smooth,
)


def _alpha_tile(rng, h, w, kind):
    yy, xx = np.mgrid[0:h, 0:w]
    if kind < 3:
        return np.full((h, w), (0, 255, int(rng.integers(40, 216)))[kind])
    if kind == 3:
        return rng.integers(0, 2, (h, w)) * 255                                                     # binary, per texel
    if kind == 4:
        return np.clip(((xx - w / 2) ** 2 + (yy - h / 2) ** 2) * (1100.0 / (h * w + 1)), 0, 255)    # soft disc
    if kind == 5:
        return rng.integers(0, 256, (h, w))                                                         # per-texel noise
    if kind == 6:
        return np.clip(6 * xx + 9 * yy + rng.integers(0, 60), 0, 255)                               # ramp into the clamp
    return np.clip(rng.integers(0, 2, (h, w)) * 255 + rng.integers(-12, 13, (h, w)), 0, 255)       # near-binary: levels clamp at both ends


ALPHA_KINDS = 8


def mosaic(h, w, seed, alpha=False, shift=0):
    """One RGBA layer: 16 x 16 tiles, tile k takes colour kind (k + shift) mod 14 and (with alpha) alpha kind (k + shift // 3) mod 8 - the two
    cycles have different lengths, so every pairing turns up in a large image.  A 4 x 4 image is the top-left block of tile 0."""
    rng = np.random.default_rng(seed)
    out = np.full((h, w, 4), 255, np.int64); k = 0
    for y0 in range(0, h, TILE):
        for x0 in range(0, w, TILE):
            th, tw = min(TILE, h - y0), min(TILE, w - x0)
            out[y0:y0 + th, x0:x0 + tw, :3] = COLOUR_KINDS[(k + shift) % len(COLOUR_KINDS)](rng, th, tw)
            if alpha:
                out[y0:y0 + th, x0:x0 + tw, 3] = _alpha_tile(rng, th, tw, (k + shift // 3) % ALPHA_KINDS)
            k += 1
    return out.astype(np.uint8)


def sequence(n, h, w, seed, alpha=False):
    """n layers: layer 0 a mosaic; every later layer keeps three quarters of the previous one's tiles (P-frame blocks that skip) and takes
    the rest from a fresh mosaic with the kinds shifted."""
    layers = [mosaic(h, w, seed, alpha)]
    for l in range(1, n):
        new = mosaic(h, w, seed + 1000 * l, alpha, shift=5 * l); cur = layers[-1].copy(); k = 0
        for y0 in range(0, h, TILE):
            for x0 in range(0, w, TILE):
                if (k + l) % 4 == 0:
                    cur[y0:y0 + TILE, x0:x0 + TILE] = new[y0:y0 + TILE, x0:x0 + TILE]
                k += 1
        layers.append(cur)
    return layers


# (name, height, width, layers, alpha): the sizes of the case table; the reference's own fixture and the 2048^2 device cases are added by the tests
SMALL_CASES = (
    ("one_block", 4, 4, 1, False), ("one_block_alpha", 4, 4, 1, True),
    ("ragged_13x7", 7, 13, 2, False), ("ragged_13x7_alpha", 7, 13, 2, True),
    ("ragged_37x50", 50, 37, 2, False), ("ragged_37x50_alpha", 50, 37, 3, True),
    ("square_52", 52, 52, 3, False), ("square_52_alpha", 52, 52, 2, True),
    ("mosaic_256", 256, 256, 5, False), ("mosaic_256_alpha", 256, 256, 5, True),
)


def case_layers(name):
    for i, (nm, h, w, n, alpha) in enumerate(SMALL_CASES):
        if nm == name:
            return sequence(n, h, w, 100 + i, alpha)
    raise KeyError(name)


def batch_layers():
    """The layers of one mixed call: six files of ONE shape (40 x 28 x 2, the ABI's rule for a call), opaque and alpha alternating, every one
    with content of its own - plus two files of other sizes and layer counts, which the call must refuse in their own slots."""
    same = [sequence(2, 28, 40, 300 + i, alpha=bool(i & 1)) for i in range(6)]
    other = [sequence(3, 20, 24, 400, alpha=False), sequence(1, 36, 52, 401, alpha=True)]
    return same, other
