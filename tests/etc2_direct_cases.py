"""Checks of the direct ETC2 RGB encode (uvol_encode_etc2_rgb_batch, csrc/tex_etc2.hip), shared by tests/test_hipemu_etc2_direct.py (the host
emulation of the kernels, no GPU) and tests/test_gpu_etc2_direct.py (the MI355X).  `mem` is material_cases.HostMem / HipMem.

The reference is the NumPy restatement below of the rule as include/uvol_codec.h states it, written from that text and vectorised over
blocks.  Texels: y_flip, replicated edges, px[4 y + x], alpha ignored.  For flip f, half h of texel (x, y) is x >= 2 (f = 0) or y >= 2
(f = 1); per half and channel m8 = (sum + 4) >> 3, q5 = (m8 * 31 + 127) // 255, q4 = (m8 * 15 + 127) // 255; a 5-bit base b expands to
(b << 3) | (b >> 2), a 4-bit base to b * 17; E(base, t) = sum over the half's texels of the smallest squared RGB error among the four
modified colours, clamped per channel.  Half search in precision P from q: step 1, t = 0 .. 7 x dd in (0, -1, +1) on all channels (clamped to
0 .. top), strictly smaller E replaces; step 2 at that table, c = 0 .. 2 x dd in (-1, +1), channel c alone from the current best base,
skipped outside 0 .. top, accepted on strictly smaller E; the unrefined result (dd = 0, first best t) is kept.  Per flip: individual = both
halves in 4 bits; differential = both halves in 5 bits, the refined pair when its deltas fit -4 .. 3, else the unrefined q5 pair when its
deltas fit, else none; differential wins when it exists and E_diff <= E_ind.  Flip 1 wins only with strictly smaller error.
Everything is bit-exact: there is no tolerance anywhere in this file."""
import numpy as np
import transcode_ref as TR

MOD = TR.ETC1_MOD                  # [table, pixel index 0 .. 3] = +small, +large, -small, -large
COUNTERS = (["differential", "individual", "flip0", "flip1"] + ["table%d" % t for t in range(8)] +
            ["refined_pair", "fallback_pair", "no_differential", "step2_move", "clamped_colour"])


def fetch_blocks(img, y_flip=1):
    """img [H, W, >= 3] uint8 -> px [by * bx, 16, 3] int64 (raster order of blocks, texel i = 4 y + x), and (by, bx)."""
    img = np.asarray(img); H, W = img.shape[:2]; by, bx = -(-H // 4), -(-W // 4)
    py = np.minimum(np.arange(by * 4), H - 1); rows = H - 1 - py if y_flip else py
    cols = np.minimum(np.arange(bx * 4), W - 1)
    v = img[rows][:, cols, :3].astype(np.int64)
    return v.reshape(by, 4, bx, 4, 3).transpose(0, 2, 1, 3, 4).reshape(by * bx, 16, 3), (by, bx)


def expand(b, top):
    return ((b << 3) | (b >> 2)) if top == 31 else b * 17


def half_err(v8, base, t):
    """v8 [n, 8, 3], base [n, 3] (8-bit), t [n] -> E [n]."""
    lv = np.clip(base[:, None, :] + MOD[t][:, :, None], 0, 255)                      # [n, idx, c]
    return ((lv[:, None, :, :] - v8[:, :, None, :]) ** 2).sum(-1).min(-1).sum(-1)


def search(v8, q, top):
    """-> refined (E, base [n, 3], t), unrefined (E, t), step-2 moves accepted [n]."""
    n = len(v8); big = np.iinfo(np.int64).max
    be = np.full(n, big); bb = np.zeros((n, 3), np.int64); bt = np.zeros(n, np.int64)
    ue = np.full(n, big); ut = np.zeros(n, np.int64)
    for t in range(8):
        tt = np.full(n, t, np.int64)
        for dd in (0, -1, 1):
            cand = np.clip(q + dd, 0, top)
            e = half_err(v8, expand(cand, top), tt)
            take = e < be
            be = np.where(take, e, be); bb = np.where(take[:, None], cand, bb); bt = np.where(take, t, bt)
            if dd == 0:
                take = e < ue
                ue = np.where(take, e, ue); ut = np.where(take, t, ut)
    moves = np.zeros(n, np.int64)
    for c in range(3):
        for dd in (-1, 1):
            nb = bb.copy(); nb[:, c] += dd
            ok = (nb[:, c] >= 0) & (nb[:, c] <= top)
            e = half_err(v8, expand(np.clip(nb, 0, top), top), bt)
            take = ok & (e < be)
            be = np.where(take, e, be); bb = np.where(take[:, None], nb, bb); moves += take
    return (be, bb, bt), (ue, ut), moves


def _fits(a, b):
    d = b - a
    return ((d >= -4) & (d <= 3)).all(1)


def encode_px(px):
    """px [n, 16, 3] -> blocks [n, 8] uint8 and the counters of COUNTERS (blocks per branch; step2_move: searches of either winner or loser)."""
    v = np.asarray(px, np.int64)[..., :3]; n = len(v)
    per_flip = []
    step2 = np.zeros(n, np.int64)
    for flip in (0, 1):
        half = np.array([(i // 4 >= 2) if flip else (i % 4 >= 2) for i in range(16)])
        r5, u5, r4, q5s = [], [], [], []
        for h in (0, 1):
            v8 = v[:, half == bool(h)]
            m8 = (v8.sum(1) + 4) >> 3; q5 = (m8 * 31 + 127) // 255; q4 = (m8 * 15 + 127) // 255
            a, b, m = search(v8, q5, 31); r5.append(a); u5.append(b); q5s.append(q5); step2 += m
            a, b, m = search(v8, q4, 15); r4.append(a); step2 += m
        e_ind = r4[0][0] + r4[1][0]
        use_ref = _fits(r5[0][1], r5[1][1]); use_fb = ~use_ref & _fits(q5s[0], q5s[1]); have = use_ref | use_fb
        d_base = [np.where(use_ref[:, None], r5[h][1], q5s[h]) for h in (0, 1)]
        d_tab = [np.where(use_ref, r5[h][2], u5[h][1]) for h in (0, 1)]
        e_diff = np.where(use_ref, r5[0][0] + r5[1][0], u5[0][0] + u5[1][0])
        diff = have & (e_diff <= e_ind)
        err = np.where(diff, e_diff, e_ind)
        base = [np.where(diff[:, None], d_base[h], r4[h][1]) for h in (0, 1)]
        tab = [np.where(diff, d_tab[h], r4[h][2]) for h in (0, 1)]
        cb = np.where(diff[:, None], (base[0] << 3) | ((base[1] - base[0]) & 7), (base[0] << 4) | base[1])
        b3 = (tab[0] << 5) | (tab[1] << 2) | np.where(diff, 2, 0) | flip
        full = [np.where(diff[:, None], expand(base[h], 31), expand(base[h], 15)) for h in (0, 1)]
        msb = np.zeros(n, np.int64); lsb = np.zeros(n, np.int64); clamped = np.zeros(n, bool)
        for h in (0, 1):
            raw = full[h][:, None, :] + MOD[tab[h]][:, :, None]
            clamped |= ((raw < 0) | (raw > 255)).any((1, 2))
        for y in range(4):
            for x in range(4):
                i = 4 * y + x; h = int(half[i])
                lv = np.clip(full[h][:, None, :] + MOD[tab[h]][:, :, None], 0, 255)
                bi = ((lv - v[:, i, None, :]) ** 2).sum(-1).argmin(-1)           # argmin: the first of equal errors
                msb |= (bi >> 1) << (4 * x + y); lsb |= (bi & 1) << (4 * x + y)
        blk = np.concatenate([cb, b3[:, None], np.stack([msb >> 8, msb & 255, lsb >> 8, lsb & 255], 1)], 1)
        per_flip.append(dict(err=err, blk=blk, diff=diff, tab=np.stack(tab, 1), refined=diff & use_ref, fallback=diff & use_fb, none=~have, clamped=clamped))
    take = per_flip[1]["err"] < per_flip[0]["err"]

    def pick(k):
        a, b = per_flip[0][k], per_flip[1][k]
        return np.where(take.reshape((n,) + (1,) * (a.ndim - 1)), b, a)
    diff, tab = pick("diff"), pick("tab")
    cnt = dict(differential=int(diff.sum()), individual=int((~diff).sum()), flip0=int((~take).sum()), flip1=int(take.sum()),
               refined_pair=int(pick("refined").sum()), fallback_pair=int(pick("fallback").sum()), no_differential=int(pick("none").sum()),
               step2_move=int((step2 > 0).sum()), clamped_colour=int(pick("clamped").sum()))
    for t in range(8):
        cnt["table%d" % t] = int((tab == t).any(1).sum())
    return pick("blk").astype(np.uint8), cnt


def encode_image(img, y_flip=1):
    px, (by, bx) = fetch_blocks(img, y_flip)
    blk, cnt = encode_px(px)
    return blk.reshape(by, bx, 8), cnt


_CACHE = {}


def reference(key, imgs, y_flip=1):
    """The rule on `imgs`, computed once per key and shared by the tests that need it (never modified)."""
    k = (key, y_flip)
    if k not in _CACHE:
        out = [encode_image(a, y_flip) for a in imgs]
        _CACHE[k] = ([o[0] for o in out], [o[1] for o in out])
        for a in _CACHE[k][0]:
            a.setflags(write=False)
    return _CACHE[k]


def block_sse(blocks, img, y_flip=1):
    """Squared RGB error per block [by * bx] of `blocks` [by, bx, 8], decoded by helpers.etc1_decode_blocks, against the texels the encoder saw."""
    import helpers
    px, (by, bx) = fetch_blocks(img, y_flip)
    dec = helpers.etc1_decode_blocks(np.asarray(blocks), bx * 4, by * 4)
    dpx, _ = fetch_blocks(dec, 0)
    return ((dpx - px) ** 2).sum((1, 2)), px


def check_properties(blocks, img, y_flip=1):
    """3.: on the bytes given: error per block <= that of transcode_ref.ref_px_etc1 on the same texels; differential blocks keep
    0 <= c5 + delta <= 31."""
    import helpers
    sse, px = block_sse(blocks, img, y_flip)
    ref, _ = TR.ref_px_etc1(np.concatenate([px, np.zeros((len(px), 16, 1), np.int64)], 2))
    by, bx = blocks.shape[:2]
    rdec, _ = fetch_blocks(helpers.etc1_decode_blocks(ref.reshape(by, bx, 8), bx * 4, by * 4), 0)
    rsse = ((rdec - px) ** 2).sum((1, 2))
    assert (sse <= rsse).all(), (np.argwhere(sse > rsse)[:4].tolist(), sse[sse > rsse][:4], rsse[sse > rsse][:4])
    b = np.asarray(blocks).reshape(-1, 8).astype(np.int64); diff = (b[:, 3] & 2) != 0
    for c in range(3):
        d = b[:, c] & 7; d = np.where(d >= 4, d - 8, d); s = (b[:, c] >> 3) + d
        assert ((s >= 0) & (s <= 31))[diff].all(), c
    return int(sse.sum()), int(rsse.sum())


# ---------------------------------------------------------------------------------------------- device runners
def run_device(cd, mem, imgs, dev_out=True):
    """imgs (one size) copied to `device` memory, encoded there, blocks read back through `mem` (dev_out) or returned as host arrays."""
    h, w = imgs[0].shape[:2]; by, bx = -(-h // 4), -(-w // 4)
    ptrs = [mem.to_dev(a) for a in imgs]
    if dev_out:
        outs = [mem.alloc(bx * by * 8) for _ in imgs]
        assert cd.encode_etc2_rgb_batch(ptrs, w, h, out_dev_ptrs=outs) is None
        got = [mem.to_host(p, np.uint8, bx * by * 8).reshape(by, bx, 8) for p in outs]
    else:
        got = cd.encode_etc2_rgb_batch(ptrs, w, h)
    mem.free_all()
    return got


def check_equal(got, want, what):
    assert len(got) == len(want)
    for k, (g, a) in enumerate(zip(got, want)):
        assert g.shape == a.shape and np.array_equal(g, a), (what, k, np.argwhere((g != a).any(-1))[:4].tolist())


def random_rgba(rng, h, w, n):
    return [rng.integers(0, 256, (h, w, 4)).astype(np.uint8) for _ in range(n)]


# ---------------------------------------------------------------------------------------------- 1. bit-exact blocks
SHAPES = ((4, 4, 1), (1, 1, 1), (5, 7, 1), (1028, 8, 2), (2048, 8, 2), (12, 12, 70))      # W, H, images


def shape_images(seed=11):
    """Noise, with a smooth ramp mixed into every other image so that low tables and the differential mode occur at every shape."""
    rng = np.random.default_rng(seed); out = []
    for (w, h, n) in SHAPES:
        imgs = random_rgba(rng, h, w, n)
        for k in range(1, n, 2):
            yy, xx = np.mgrid[0:h, 0:w]
            ramp = np.stack([(3 * xx + 5 * yy + 17 * k) % 256, (2 * xx + yy + 40 * k) % 256, (xx + 7 * yy + 90 * k) % 256, 255 + 0 * xx], -1)
            imgs[k] = np.clip(ramp + rng.integers(-6, 7, ramp.shape), 0, 255).astype(np.uint8)
        out.append(imgs)
    return out


def run_shapes(cd, mem, y_flip=1):
    """One block; replication in both axes; partial blocks on the scalar fetch path; aligned rows with a block count that is no multiple of
    the workgroup; the workload's row length; more images than a wave has lanes.  cd was created with the same y_flip."""
    for (w, h, n), imgs in zip(SHAPES, shape_images()):
        want, _ = reference(("shape", w, h, n), imgs, y_flip)
        got = run_device(cd, mem, imgs)
        check_equal(got, want, (w, h, n, y_flip))
        for g, a in zip(got, imgs):                       # 3.: the properties on the device's own bytes, every block
            check_properties(g, a, y_flip)


def run_grid_stride(cd, mem, layers=9, reps=256):
    """More blocks than one round of the kernel's grid-stride loop takes on the device (32768 workgroups of 64 blocks): `layers` images of
    2048 x (8 reps), each one of the two 2048 x 8 images of test 1 repeated downwards - so the rule's blocks are those of test 1, repeated
    (a whole number of block rows, also under y_flip) - 2 359 296 blocks at the defaults.  (The emulation build strides after 4 workgroups,
    so there every shape of test 1 runs the later rounds.)"""
    tiles = shape_images()[4]; want, _ = reference(("shape", 2048, 8, 2), tiles)
    assert tiles[0].shape == (8, 2048, 4) and layers * 512 * 2 * reps > 32768 * 64
    imgs = [np.tile(tiles[k % 2], (reps, 1, 1)) for k in range(layers)]
    got = run_device(cd, mem, imgs)
    for k, g in enumerate(got):
        assert np.array_equal(g, np.tile(want[k % 2], (reps, 1, 1))), k


# ---------------------------------------------------------------------------------------------- 2. constructed content
def constructed_image(seed=12):
    """One image of 4x4 cells, each built for a branch of the rule (see the list in the body).  [H, W, 4] with W = 256."""
    rng = np.random.default_rng(seed); cells = []

    def flat(c):
        a = np.empty((4, 4, 3), np.int64); a[:] = c; return a
    for _ in range(192):                                                         # uniform noise
        cells.append(rng.integers(0, 256, (4, 4, 3)))
    for k in range(128):                                                         # smooth ramps, every slope and direction
        yy, xx = np.mgrid[0:4, 0:4]; s = rng.integers(-9, 10, (3, 2)); o = rng.integers(0, 256, 3)
        cells.append(np.clip(np.stack([o[c] + s[c, 0] * xx + s[c, 1] * yy for c in range(3)], -1), 0, 255))
    for k in range(192):                                                         # split left / right and top / bottom into two flat colours
        a, b = rng.integers(0, 256, 3), rng.integers(0, 256, 3)
        if k % 3 == 0:
            b = np.clip(a + rng.integers(-30, 31, 3), 0, 255)                    # (near colours: differential)
        c = flat(a)
        if k & 1: c[:, 2:] = b
        else: c[2:] = b
        cells.append(c)
    cells += [flat(0), flat(255), flat((0, 255, 0)), flat((255, 0, 255))]        # all 0, all 255 (and per channel)
    for _ in range(60):                                                          # only 0 and 255 texels: clamping under the large tables
        cells.append(255 * rng.integers(0, 2, (4, 4, 1)) * np.ones((1, 1, 3), np.int64))
    for _ in range(64):                                                          # ... per channel
        cells.append(255 * rng.integers(0, 2, (4, 4, 3)))
    for d in (3, 4, -4, -5):                                                     # half pairs whose q5 differ by exactly d in one channel
        for k in range(24):
            ch = k % 3; q = rng.integers(6, 26, 3); q2 = q.copy(); q2[ch] += d
            c = flat(expand(q, 31)); b = expand(q2, 31)
            if k & 1: c[:, 2:] = b
            else: c[2:] = b
            if k >= 12:                                                          # the same with noise: the refined pair may leave -4 .. 3
                c = np.clip(c + rng.integers(-12, 13, c.shape), 0, 255)
            cells.append(c)
    for _ in range(256):                                                         # noisy halves about 3 .. 4 steps of q5 apart in every channel
        q = rng.integers(5, 26, 3); dq = rng.choice((-4, -3, 3), 3); amp = int(rng.integers(4, 40))
        c = flat(expand(q, 31)); b = expand(q + dq, 31)
        if rng.integers(0, 2): c[:, 2:] = b
        else: c[2:] = b
        cells.append(np.clip(c + rng.integers(-amp, amp + 1, c.shape), 0, 255))
    while len(cells) % 64:
        cells.append(flat(128))
    rows = len(cells) // 64
    img = np.zeros((rows * 4, 256, 4), np.uint8); img[..., 3] = 255
    for k, c in enumerate(cells):
        img[4 * (k // 64):4 * (k // 64) + 4, 4 * (k % 64):4 * (k % 64) + 4, :3] = c
    return img


def constructed_reference():
    """Blocks and counters of the constructed image; every counter must be > 0 (asserted on the CPU, before any device is consulted)."""
    img = constructed_image()
    (want,), (cnt,) = reference("constructed", [img])
    assert sorted(cnt) == sorted(COUNTERS)
    assert all(cnt[k] > 0 for k in COUNTERS), cnt
    return img, want, cnt


def run_constructed(cd, mem):
    img, want, cnt = constructed_reference()
    got = run_device(cd, mem, [img])
    check_equal(got, [want], "constructed")
    check_properties(got[0], img)
    return cnt


# ---------------------------------------------------------------------------------------------- 4. against today's target
def run_against_transcode(cd, mem):
    """64 x 64, 3 layers of the texture generator cli_helpers.make_sequence uses: RGB PSNR of the direct blocks against the source >= that of
    the ETC1 transcode of the ETC1S encode of the same layers (both computed here); a constant image is the same texels on both paths."""
    import helpers, synth
    tex = synth.texture_sequence(3, size=64, seed=3)

    def psnr(blocks, src, flipped):
        dec = helpers.etc1_decode_blocks(np.asarray(blocks), 64, 64)[..., :3].astype(np.float64)
        s = src[::-1] if flipped else src
        mse = ((dec - s[..., :3].astype(np.float64)) ** 2).mean()
        return 10 * np.log10(255.0 ** 2 / mse) if mse else np.inf
    direct = cd.encode_etc2_rgb_batch(tex, 64, 64)
    trans = cd.transcode_texture_segments_etc1([cd.encode_texture_segment(tex)])[0]
    for l in range(3):                                   # (y_flip = 1: both paths store the bottom row first)
        pd, pt = psnr(direct[l], tex[l], True), psnr(trans[l], tex[l], True)
        print("layer %d: direct %.2f dB, transcoded from ETC1S %.2f dB" % (l, pd, pt))
        assert pd >= pt, (l, pd, pt)
    const = np.empty((64, 64, 4), np.uint8); const[:] = (90, 140, 200, 255)
    d = cd.encode_etc2_rgb_batch([const] * 3, 64, 64)
    t = cd.transcode_texture_segments_etc1([cd.encode_texture_segment([const] * 3)])[0]
    for l in range(3):
        assert np.array_equal(helpers.etc1_decode_blocks(d[l], 64, 64), helpers.etc1_decode_blocks(t[l], 64, 64))


# ---------------------------------------------------------------------------------------------- 5. sources and sinks
def mem_fill(mem, ptr, nbytes):
    """Zero a `device` buffer between two checks that write the same bytes to it."""
    import ctypes as C
    if hasattr(mem, "hip"):
        assert mem.hip.hipMemset(C.c_void_p(ptr), 0, C.c_size_t(nbytes)) == 0
    else:
        C.memset(ptr, 0, nbytes)


def run_sources_and_sinks(cd, mem, png_scanlines, arena):
    """Layers of an ingest slot (7 x 13, three images, sync=False), of a downscale slot; host inputs as arrays and as bytes; device outputs
    through `mem`; an output in uvol_host_alloc memory (`arena`: a uvol.PinnedArena).  Every combination gives the rule's bytes."""
    import downscale_cases as DC
    rng = np.random.default_rng(13); w, h = 7, 13
    imgs = random_rgba(rng, h, w, 3)
    want, _ = reference("ingest 7x13", imgs)
    lay = cd.unfilter_png_batch_dev([png_scanlines(a, rng) for a in imgs], w, h, 4, slot=1, sync=False)
    assert lay[1] - lay[0] == w * h * 4 and (lay[1] & 15) != 0
    check_equal(cd.encode_etc2_rgb_batch(lay, w, h), want, "ingest slot -> host")
    lay = cd.unfilter_png_batch_dev([png_scanlines(a, rng) for a in imgs], w, h, 4, slot=0, sync=False)
    outs = [mem.alloc(2 * 4 * 8) for _ in imgs]
    cd.encode_etc2_rgb_batch(lay, w, h, out_dev_ptrs=outs)
    check_equal([mem.to_host(p, np.uint8, 64).reshape(4, 2, 8) for p in outs], want, "ingest slot -> device")
    # a downscale slot: 22 x 10 by 2 -> 11 x 5
    big = random_rgba(rng, 10, 22, 2); small = [DC.downscale(a, 2) for a in big]
    swant, _ = reference("downscale 11x5", small)
    sl = cd.downscale_rgba_batch_dev(big, 22, 10, 2, slot=1, on_device=False)
    check_equal(cd.encode_etc2_rgb_batch(sl, 11, 5), swant, "downscale slot -> host")
    souts = [mem.alloc(3 * 2 * 8) for _ in small]
    cd.encode_etc2_rgb_batch(sl, 11, 5, out_dev_ptrs=souts)
    check_equal([mem.to_host(p, np.uint8, 48).reshape(2, 3, 8) for p in souts], swant, "downscale slot -> device")
    # host inputs as arrays and as bytes, to host and to device outputs
    check_equal(cd.encode_etc2_rgb_batch(imgs, w, h), want, "host arrays -> host")
    check_equal(cd.encode_etc2_rgb_batch([a.tobytes() for a in imgs], w, h), want, "host bytes -> host")
    for form, src in (("arrays", imgs), ("bytes", [a.tobytes() for a in imgs])):
        cd.encode_etc2_rgb_batch(src, w, h, out_dev_ptrs=outs)
        check_equal([mem.to_host(p, np.uint8, 64).reshape(4, 2, 8) for p in outs], want, "host %s -> device" % form)
        for p in outs:
            mem_fill(mem, p, 64)
    # outputs in uvol_host_alloc memory (all of them: the direct DMA path), from host inputs, device inputs, an ingest slot and a downscale slot
    import ctypes as C
    pin = [arena.take((64,), np.uint8) for _ in imgs]

    def to_pinned(src, dev, n, pw, ph, nbytes, shape, expect, what):
        for p in pin: p[:] = 0
        ptrs = (C.c_void_p * n)(*[(a.ctypes.data if not dev else a) for a in src]); op = (C.c_void_p * n)(*[p.ctypes.data for p in pin[:n]])
        rc = cd.L.uvol_encode_etc2_rgb_batch(cd.h, ptrs, n, pw, ph, 1 if dev else 0, op, nbytes, 0)
        assert rc == 0, cd.error()
        check_equal([p[:nbytes].reshape(shape) for p in pin[:n]], expect, what + " -> uvol_host_alloc memory")
    to_pinned(imgs, False, 3, w, h, 64, (4, 2, 8), want, "host arrays")
    to_pinned([mem.to_dev(a) for a in imgs], True, 3, w, h, 64, (4, 2, 8), want, "device layers")
    lay = cd.unfilter_png_batch_dev([png_scanlines(a, rng) for a in imgs], w, h, 4, slot=1, sync=False)
    to_pinned(lay, True, 3, w, h, 64, (4, 2, 8), want, "ingest slot")
    sl = cd.downscale_rgba_batch_dev(big, 22, 10, 2, slot=0, on_device=False)
    to_pinned(sl, True, 2, 11, 5, 48, (2, 3, 8), swant, "downscale slot")
    mem.free_all()


# ---------------------------------------------------------------------------------------------- 6. refusals
def run_refusals(cd, mem, UvolError):
    """Every refusal names its argument and leaves the outputs untouched; a later valid call on the same context succeeds."""
    rng = np.random.default_rng(14)
    img = random_rgba(rng, 8, 8, 1)[0]; p = mem.to_dev(img)
    mark = np.full(32, 0xA5, np.uint8)
    o = mem.to_dev(mark); o2 = mem.to_dev(mark)

    def untouched():
        assert (mem.to_host(o, np.uint8, 32) == 0xA5).all() and (mem.to_host(o2, np.uint8, 32) == 0xA5).all()

    def refused(code, word, *args, **kw):
        try:
            cd.encode_etc2_rgb_batch(*args, **kw)
        except UvolError as e:
            assert ("rc=%d" % code) in str(e) and word in str(e), (word, str(e))
            untouched(); return
        raise AssertionError("not refused: " + word)
    refused(-1, "rgba[1]", [p, 0], 8, 8, on_device=True, out_dev_ptrs=[o, o2])
    refused(-1, "rgba[0]", [None, img], 8, 8, on_device=False, out_dev_ptrs=[o, o2])
    refused(-1, "blocks[1]", [p, p], 8, 8, out_dev_ptrs=[o, 0])
    refused(-1, "rgba[1]", [p, p + 2], 8, 8, on_device=True, out_dev_ptrs=[o, o2])
    refused(-1, "blocks[0]", [p], 8, 8, out_dev_ptrs=[o + 4])
    for (w, h) in ((0, 8), (8, 0), (8193, 1), (1, 16385)):
        refused(-1, "width", [p], w, h, on_device=True, out_dev_ptrs=[o])
    refused(-4, "layer_cap", [p], 8, 8, out_dev_ptrs=[o], layer_cap=31)
    # the same refusals with HOST outputs: the caller's arrays stay as they were
    import ctypes as C
    host = [np.full(32, 0x5A, np.uint8) for _ in range(2)]

    def host_call(layers, n, w, h, dev, outs, cap):
        rc = cd.L.uvol_encode_etc2_rgb_batch(cd.h, (C.c_void_p * max(n, 1))(*layers), n, w, h, dev, (C.c_void_p * max(n, 1))(*outs), cap, 0)
        assert all((a == 0x5A).all() for a in host), "a refused call wrote to a host output"
        return rc
    hp = [a.ctypes.data for a in host]
    assert host_call([p, None], 2, 8, 8, 1, hp, 32) == -1 and "rgba[1]" in cd.error()
    assert host_call([p, p], 2, 8, 8, 1, [hp[0], None], 32) == -1 and "blocks[1]" in cd.error()
    assert host_call([p, p + 2], 2, 8, 8, 1, hp, 32) == -1 and "rgba[1]" in cd.error()
    assert host_call([img.ctypes.data, None], 2, 8, 8, 0, hp, 32) == -1 and "rgba[1]" in cd.error()
    for (w, h) in ((0, 8), (8, 0), (8193, 1), (1, 16385)):
        assert host_call([p], 1, w, h, 1, hp[:1], 1 << 30) == -1 and "width" in cd.error()
    assert host_call([p], 1, 8, 8, 1, hp[:1], 31) == -4 and "layer_cap" in cd.error()
    assert host_call([p], 0, 8, 8, 1, hp[:1], 32) == 0
    assert cd.encode_etc2_rgb_batch([], 8, 8, out_dev_ptrs=[]) is None           # n = 0: UVOL_OK, nothing happens
    assert cd.encode_etc2_rgb_batch([], 0, 0) == []
    untouched()
    assert cd.L.uvol_etc2_rgb_bound(8, 8) == 32 and cd.L.uvol_etc2_rgb_bound(5, 7) == 32 and cd.L.uvol_etc2_rgb_bound(1, 1) == 8
    cd.encode_etc2_rgb_batch([p], 8, 8, out_dev_ptrs=[o])                        # the context still works
    want, _ = reference("refusals 8x8", [img])
    check_equal([mem.to_host(o, np.uint8, 32).reshape(2, 2, 8)], want, "after the refusals")
    mem.free_all()


def run_profile_group(cd):
    """The entry point registers a profile group of its own."""
    cd.profile(True); cd.profile_reset()
    cd.encode_etc2_rgb_batch([np.zeros((4, 4, 4), np.uint8)], 4, 4)
    rep = cd.profile_report(); cd.profile(False)
    assert [r["launches"] for r in rep if r["name"] == "etc2.encode"] == [1], rep


# ---------------------------------------------------------------------------------------------- 7. driver
def run_driver(exe, root, uastc=False):
    """7 frames of 32 x 32 in segments of 3: `--targets ktx2,etc2 --etc2-direct` writes the .ktx2 files and uvol.json of the run without the
    flag, and .etc2 files that are the rule on the source images (the driver's y_flip = 1); with --uastc the same (the etc2 target is only
    allowed there WITH the flag); with --texture-ladder 2 --etc2-scale 2 the rule on the NumPy-downscaled images."""
    import os, subprocess
    import cli_helpers
    import downscale_cases as DC
    cfgp, cfg, meshes, texs = cli_helpers.make_sequence(root, n_frames=7, tex=32, batch=3)
    out = cfg["OutputDirectory"]

    def run(extra, ok=True):
        r = subprocess.run([exe, cfgp, "--batch-frames", "3"] + extra, cwd=root, capture_output=True, text=True, timeout=900)
        assert (r.returncode == 0) == ok, r.stdout + r.stderr
        return r

    def tree():
        return {os.path.relpath(os.path.join(d, f), out): open(os.path.join(d, f), "rb").read() for d, _, fs in os.walk(out) for f in fs}

    def check_etc2(files, imgs, size):
        want, _ = reference(("driver", size), imgs)
        for k in range(7):
            raw = np.frombuffer(files["texture_etc2_baseColor_default/%05d.etc2" % k], np.uint8)
            assert raw.size == (size // 4) ** 2 * 8
            assert np.array_equal(raw.reshape(size // 4, size // 4, 8), want[k]), k
    mode = ["--uastc"] if uastc else []
    if uastc:
        b = run(mode + ["--targets", "ktx2,etc2"], ok=False)
        assert "❌" in b.stdout
        base = None
        run(mode + ["--targets", "ktx2"]); plain = tree()          # (the etc2 target without the flag is refused there: the run without the target)
    else:
        run(["--targets", "ktx2,etc2"]); base = tree()
    run(mode + ["--targets", "ktx2,etc2", "--etc2-direct"]); got = tree()
    if base is not None:
        assert sorted(got) == sorted(base)
        for name in base:
            if not name.endswith(".etc2"):
                assert got[name] == base[name], name
        assert any(got[n] != base[n] for n in base if n.endswith(".etc2"))
    else:
        assert sorted(n for n in got if not n.endswith(".etc2")) == sorted(plain) and any(n.endswith(".ktx2") for n in plain)
        for name in plain:
            if name != "uvol.json":                              # (the manifest lists the etc2 target)
                assert got[name] == plain[name], name
    check_etc2(got, texs, 32)
    run(mode + ["--targets", "ktx2,etc2", "--texture-ladder", "2", "--etc2-scale", "2", "--etc2-direct"]); lgot = tree()
    for name, data in (base if base is not None else plain).items():      # the full-size segments and the geometry are those of the run without the ladder
        if not name.endswith(".etc2") and name != "uvol.json":
            assert lgot[name] == data, name
    check_etc2(lgot, [DC.downscale(t, 2) for t in texs], 16)
