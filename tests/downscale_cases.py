"""Checks of the device downscale (uvol_downscale_rgba_batch_dev, csrc/tex_downscale.hip), shared by tests/test_hipemu_downscale.py (the host
emulation of the kernels, no GPU) and tests/test_gpu_downscale.py (the MI355X).  `mem` is material_cases.HostMem / HipMem: how "device"
memory is written and read back.

The reference is the NumPy restatement below of the filter as include/uvol_codec.h defines it, written from that text: for a factor f in
{2, 4, 8}, W x H becomes ceil(W / f) x ceil(H / f); output texel (X, Y) comes in one step from the box B of the n input texels with
f X <= x < min(f X + f, W), f Y <= y < min(f Y + f, H):
  lin[v] = floor(65535 L(v / 255) + 0.5), L = the sRGB decoding function, in double;
  A = sum a, out.a = (2 A + n) // (2 n);
  per colour channel: N = sum lin[c] a, D = A (when A == 0: N = sum lin[c], D = n); m = (2 N + D) // (2 D); out.c = the v with the smallest
  |lin[v] - m|, the lower v at a tie.
Everything is bit-exact: there is no tolerance anywhere in this file."""
import numpy as np

FACTORS = (2, 4, 8)


def lin_table():
    s = np.arange(256, dtype=np.float64) / 255.0
    L = np.where(s <= 0.04045, s / 12.92, ((s + 0.055) / 1.055) ** 2.4)
    return np.floor(65535.0 * L + 0.5).astype(np.int64)


LIN = lin_table()


def check_table():
    """What the definition states about the table: strictly increasing with smallest step 19, no entry near a rounding boundary, three values."""
    s = np.arange(256, dtype=np.float64) / 255.0
    x = 65535.0 * np.where(s <= 0.04045, s / 12.92, ((s + 0.055) / 1.055) ** 2.4) + 0.5
    assert np.abs(x - np.round(x)).min() > 0.0016
    assert np.diff(LIN).min() == 19
    assert (LIN[0], LIN[1], LIN[254], LIN[255]) == (0, 20, 64952, 65535)
    assert int(np.sum((np.diff(LIN) % 2) == 0)) == 122          # steps with a reachable tie half way


def downscale(img, f):
    """img [H, W, 4] uint8 -> [ceil(H / f), ceil(W / f), 4] uint8."""
    img = np.asarray(img); H, W = img.shape[:2]; oh, ow = -(-H // f), -(-W // f)
    px = np.zeros((oh * f, ow * f, 4), np.int64); px[:H, :W] = img
    inside = np.zeros((oh * f, ow * f), np.int64); inside[:H, :W] = 1

    def box(a):
        return a.reshape((oh, f, ow, f) + a.shape[2:]).sum(axis=(1, 3))
    n = box(inside)
    a = px[..., 3] * inside; A = box(a)
    lin = LIN[px[..., :3]] * inside[..., None]
    Nw, Nu = box(lin * a[..., None]), box(lin)
    clear = A == 0
    N = np.where(clear[..., None], Nu, Nw); D = np.where(clear, n, A)[..., None]
    m = (2 * N + D) // (2 * D)
    assert int((2 * N + D).max()) <= 2139078720
    out = np.empty((oh, ow, 4), np.uint8)
    out[..., :3] = np.abs(LIN[None, None, None, :] - m[..., None]).argmin(-1)       # argmin: the first, i.e. the lowest v, of equal distances
    out[..., 3] = (2 * A + n) // (2 * n)
    return out


def read_layers(mem, ptrs, w, h, f):
    oh, ow = -(-h // f), -(-w // f)
    return [mem.to_host(p, np.uint8, oh * ow * 4).reshape(oh, ow, 4) for p in ptrs]


def run_device(cd, mem, imgs, f, slot=0):
    """imgs (one size) copied to `device` memory, downscaled there, read back."""
    h, w = imgs[0].shape[:2]
    ptrs = [mem.to_dev(a) for a in imgs]
    out = cd.downscale_rgba_batch_dev(ptrs, w, h, f, slot=slot)
    got = read_layers(mem, out, w, h, f)
    mem.free_all()
    return got


def check_equal(got, imgs, f, what):
    for k, (g, a) in enumerate(zip(got, imgs)):
        want = downscale(a, f)
        assert g.shape == want.shape and np.array_equal(g, want), (what, f, k, np.argwhere(g != want)[:4].tolist())


def random_rgba(rng, h, w, n):
    return [rng.integers(0, 256, (h, w, 4)).astype(np.uint8) for _ in range(n)]


# ---------------------------------------------------------------------------------------------- 1. bit-exact layers
SHAPES = ((1, 1, 1), (1, 9, 1), (9, 1, 1), (1028, 20, 2), (2048, 8, 2), (12, 12, 70))      # W, H, images


def run_shapes(cd, mem, seed=5):
    """Device inputs: boxes of one texel, of 8 rows and of 1 row; an output width of 257 (a tail behind the 16-byte path); the aligned
    path at the workload's row length; more images than a wave has lanes."""
    rng = np.random.default_rng(seed)
    for (w, h, n) in SHAPES:
        imgs = random_rgba(rng, h, w, n)
        for f in FACTORS:
            check_equal(run_device(cd, mem, imgs, f, slot=f & 1), imgs, f, (w, h, n))


def run_ingest_slot(cd, mem, png_scanlines, seed=6):
    """7 x 13, three images through uvol_unfilter_png_batch_dev: the second and third layer of the ingest slot start 4-byte aligned only, and the
    downscale orders itself behind the un-filter (sync=False)."""
    rng = np.random.default_rng(seed); w, h = 7, 13
    imgs = random_rgba(rng, h, w, 3)
    for f in FACTORS:
        lay = cd.unfilter_png_batch_dev([png_scanlines(a, rng) for a in imgs], w, h, 4, slot=1, sync=False)
        assert lay[1] - lay[0] == w * h * 4 and (lay[1] & 15) != 0
        out = cd.downscale_rgba_batch_dev(lay, w, h, f, slot=0)
        check_equal(read_layers(mem, out, w, h, f), imgs, f, "ingest slot")


def run_host_inputs(cd, mem, seed=7):
    rng = np.random.default_rng(seed); w, h = 1028, 20
    imgs = random_rgba(rng, h, w, 2)
    for f in FACTORS:
        out = cd.downscale_rgba_batch_dev(imgs, w, h, f, slot=1, on_device=False)
        check_equal(read_layers(mem, out, w, h, f), imgs, f, "host inputs")
    out = cd.downscale_rgba_batch_dev([a.tobytes() for a in imgs], w, h, 2)
    check_equal(read_layers(mem, out, w, h, 2), imgs, 2, "host inputs as bytes")


# ---------------------------------------------------------------------------------------------- 2. arithmetic edges
def run_arithmetic_edges(cd, mem):
    rng = np.random.default_rng(8)
    for f in FACTORS:
        # the largest sums
        full = np.full((16, 24, 4), 255, np.uint8)
        got = run_device(cd, mem, [full], f)
        check_equal(got, [full], f, "all 255"); assert (got[0] == 255).all()
        # a constant image maps to itself (odd size: boxes cut by both borders)
        for c in ((0, 0, 0, 0), (1, 2, 3, 4), (200, 100, 50, 255), (13, 77, 254, 1), (9, 8, 7, 0)):
            const = np.empty((11, 19, 4), np.uint8); const[:] = c
            got = run_device(cd, mem, [const], f)
            check_equal(got, [const], f, "constant"); assert (got[0] == np.array(c, np.uint8)).all(), (f, c)
        # a box whose alpha is all zero: the plain mean in linear light, alpha 0
        clear = rng.integers(0, 256, (16, 16, 4)).astype(np.uint8); clear[..., 3] = 0
        got = run_device(cd, mem, [clear], f)
        check_equal(got, [clear], f, "alpha all zero"); assert (got[0][..., 3] == 0).all()
    # 2 x 2 black / white opaque checker: 188 (a byte average would give 128)
    chk = np.zeros((8, 8, 4), np.uint8); chk[..., 3] = 255; chk[0::2, 1::2, :3] = 255; chk[1::2, 0::2, :3] = 255
    for f in FACTORS:
        got = run_device(cd, mem, [chk], f)
        check_equal(got, [chk], f, "checker"); assert (got[0] == np.array((188, 188, 188, 255), np.uint8)).all(), got[0][0, 0]
    # one opaque texel beside three transparent ones of another colour: the colour does not bleed, alpha is the mean
    tn = np.empty((4, 6, 4), np.uint8); tn[:] = (0, 255, 0, 0); tn[0::2, 0::2] = (200, 100, 50, 255)
    got = run_device(cd, mem, [tn], 2)
    check_equal(got, [tn], 2, "transparent neighbour"); assert (got[0] == np.array((200, 100, 50, 64), np.uint8)).all(), got[0][0, 0]
    # every grey level averaged with its neighbour: m lies half way between lin[v] and lin[v + 1]; an even step is a tie and gives v, an odd
    # one rounds m up and gives v + 1 (the inverse search, both outcomes at every v)
    pairs = np.empty((2 * 255, 2, 4), np.uint8); pairs[..., 3] = 255
    v = np.repeat(np.arange(255), 2)
    pairs[:, 0, :3] = v[:, None]; pairs[:, 1, :3] = v[:, None] + 1
    got = run_device(cd, mem, [pairs], 2)
    check_equal(got, [pairs], 2, "grey pairs")
    step = np.diff(LIN)
    assert np.array_equal(got[0][:, 0, 0], np.arange(255) + (step % 2 == 1)) and (got[0][:, 0, 3] == 255).all()


# ---------------------------------------------------------------------------------------------- 3. into the encoder
def run_into_encoder(O, cd, mem, uastc=False):
    """Layers of synth.texture_sequence(2, size=64), downscaled by 2 on the device and handed to the encoder from there = the oracle
    encoder's bytes for the NumPy-downscaled images.  cd: a context created with uastc=1 when `uastc`."""
    import synth
    tex = synth.texture_sequence(2, size=64)
    out = cd.downscale_rgba_batch_dev([mem.to_dev(t) for t in tex], 64, 64, 2)
    got = cd.encode_texture_segment_dev(out, 32, 32)
    mem.free_all()
    small = [downscale(t, 2) for t in tex]
    assert got == (O.uastc_ktx2_encode(small) if uastc else O.ktx2_encode(small))


# ---------------------------------------------------------------------------------------------- 4. slots and errors
def run_slots(cd, mem):
    rng = np.random.default_rng(9)
    a = random_rgba(rng, 10, 14, 2); b = random_rgba(rng, 22, 6, 3)
    pa = cd.downscale_rgba_batch_dev([mem.to_dev(x) for x in a], 14, 10, 2, slot=0)
    pb = cd.downscale_rgba_batch_dev([mem.to_dev(x) for x in b], 6, 22, 4, slot=1)
    check_equal(read_layers(mem, pb, 6, 22, 4), b, 4, "slot 1")
    check_equal(read_layers(mem, pa, 14, 10, 2), a, 2, "slot 0 after slot 1 was written")
    # uvol_trim gives the slots back; the next call allocates again
    cd.trim()
    pa = cd.downscale_rgba_batch_dev([mem.to_dev(x) for x in a], 14, 10, 8, slot=0)
    check_equal(read_layers(mem, pa, 14, 10, 8), a, 8, "after uvol_trim")
    assert cd.downscale_rgba_batch_dev([], 14, 10, 2) == []            # n <= 0: UVOL_OK, nothing happens
    assert cd.downscale_rgba_batch_dev([], 0, 0, 3, slot=5) == []
    mem.free_all()


def run_refusals(cd, mem, UvolError):
    """Every refusal is UVOL_E_INVALID (-1) and names the argument."""
    img = np.zeros((4, 4, 4), np.uint8); p = mem.to_dev(img)

    def refused(word, *args, **kw):
        try:
            cd.downscale_rgba_batch_dev(*args, **kw)
        except UvolError as e:
            assert "rc=-1" in str(e) and word in str(e), (word, str(e))
            return
        raise AssertionError("not refused: " + word)
    for f in (0, 1, 3, 5, 6, 16, -2):
        refused("factor", [p], 4, 4, f)
    for s in (-1, 2):
        refused("slot", [p], 4, 4, 2, slot=s)
    refused("rgba[1]", [p, 0], 4, 4, 2, on_device=True)
    refused("rgba[0]", [None, img], 4, 4, 2, on_device=False)
    for (w, h) in ((0, 4), (4, 0), (8193, 1), (1, 16385)):
        refused("width", [p], w, h, 2, on_device=True)
    refused("height", [p], 1, 16385, 2, on_device=True)
    got = cd.downscale_rgba_batch_dev([p], 4, 4, 2)                    # the context still works
    assert (read_layers(mem, got, 4, 4, 2)[0] == 0).all()
    mem.free_all()


# ---------------------------------------------------------------------------------------------- 5. driver plumbing
def run_driver(O, exe, root, ktx2_info, baseline_exe=None):
    """`uvolenc --texture-ladder 2,4 --targets ktx2,etc2 --etc2-scale 2` on a tiny project (16 x 16 PNGs, 5 frames in segments of 3: a short
    last segment): directories, file counts, the rungs' files, the manifest, the player's choice, the etc2 tier."""
    import json, os, subprocess
    import cli_helpers, player_urls
    cfgp, cfg, meshes, texs = cli_helpers.make_sequence(root, n_frames=5, tex=16, batch=3)
    r = subprocess.run([exe, cfgp, "--batch-frames", "3", "--texture-ladder", "2,4", "--targets", "ktx2,etc2", "--etc2-scale", "2"],
                       cwd=root, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    out = cfg["OutputDirectory"]
    full = [open(os.path.join(out, "texture_ktx2_baseColor_default", "%05d.ktx2" % s), "rb").read() for s in range(2)]
    assert sorted(os.listdir(os.path.join(out, "texture_ktx2_baseColor_default"))) == ["00000.ktx2", "00001.ktx2"]
    for s, n in enumerate([3, 2]):
        assert full[s] == O.ktx2_encode(texs[3 * s:3 * s + n])           # the full-size target is what it was
    for f, size in ((2, 8), (4, 4)):
        d = os.path.join(out, "texture_ktx2_%dx%d_baseColor_default" % (size, size))
        assert sorted(os.listdir(d)) == ["00000.ktx2", "00001.ktx2"]
        for s, n in enumerate([3, 2]):
            data = open(os.path.join(d, "%05d.ktx2" % s), "rb").read()
            assert ktx2_info(data) == (size, size, n)
            small = [downscale(t, f) for t in texs[3 * s:3 * s + n]]
            # The existing driver tests gate the full-size files by the oracle encoder's BYTES (none of them uses a PSNR figure), so the rungs
            # are held to the same, on the NumPy-downscaled source.  The decode against that source (stored rows are bottom-up) must then be
            # no worse than the reference codec's own error on it: the gate is the PSNR of the oracle's encode + decode of the same images,
            # computed here (ETC1S at 8 x 8 and 4 x 4 texels is four blocks and one: 22 - 24 dB on this content, whoever encodes it).
            want = O.ktx2_encode(small)
            assert data == want, (f, s)
            dec, ref = O.ktx2_decode(data), O.ktx2_decode(want)
            for l in range(n):
                q, gate = O.psnr(dec.images[l], small[l][::-1]), O.psnr(ref.images[l], small[l][::-1])
                print("rung 1/%d segment %d layer %d: %.2f dB (the reference codec: %.2f dB)" % (f, s, l, q, gate))
                assert q >= gate, (f, s, l, q, gate)
    man = json.load(open(os.path.join(out, "uvol.json")))
    T = man["texture"]["targets"]
    assert list(T) == ["ktx2", "etc2", "ktx2_8x8", "ktx2_4x4"]
    assert T["ktx2"]["resolution"] == [16, 16] and T["etc2"]["resolution"] == [8, 8]
    for name, size in (("ktx2_8x8", 8), ("ktx2_4x4", 4)):
        t = T[name]
        assert (t["format"], t["resolution"], t["sequenceSize"], t["sequenceCount"], t["frameRate"]) == ("ktx2", [size, size], 3, 2, T["ktx2"]["frameRate"])
        assert (t["type"], t["tag"]) == ("baseColor", "default")
    for supports, want in ((False, "ktx2"), (True, "etc2")):
        urls = player_urls.resolve(os.path.join(out, "uvol.json"), supports_etc2=supports)
        assert urls["textureTarget"] == want
        for rel in urls["geometry"] + urls["texture"]:
            assert os.path.isfile(os.path.join(out, rel)), rel
    assert urls["resolution"] == [8, 8] and len(urls["texture"]) == 5
    # the etc2 tier is transcoded from the rung's segments: ceil(w / 4) ceil(h / 4) 8 bytes, and decodes to that rung's RGBA decode
    import helpers
    for k, rel in enumerate(urls["texture"]):
        raw = np.frombuffer(open(os.path.join(out, rel), "rb").read(), np.uint8)
        assert raw.size == 2 * 2 * 8
        ref = O.ktx2_decode(open(os.path.join(out, "texture_ktx2_8x8_baseColor_default", "%05d.ktx2" % (k // 3)), "rb").read())
        assert np.array_equal(helpers.etc1_decode_blocks(raw.reshape(2, 2, 8), 8, 8), ref.images[k % 3])
    # bad flag values: a message and exit 1, nothing written
    for extra in (["--texture-ladder", "3"], ["--texture-ladder", "2", "--targets", "ktx2,etc2", "--etc2-scale", "4"], ["--etc2-scale", "2"]):
        b = subprocess.run([exe, cfgp] + extra, cwd=root, capture_output=True, text=True, timeout=900)
        assert b.returncode == 1 and "❌" in b.stdout, (extra, b.stdout)
    return out


def run_driver_default_unchanged(exe, root):
    """The same project WITHOUT the new flags: the file list and the manifest are what the driver wrote before this feature (the names and the
    manifest text below are the parent commit's output for this project)."""
    import json, os, subprocess
    import cli_helpers
    cfgp, cfg, meshes, texs = cli_helpers.make_sequence(root, n_frames=5, tex=16, batch=3)
    r = subprocess.run([exe, cfgp, "--batch-frames", "3", "--targets", "ktx2,etc2"], cwd=root, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    out = cfg["OutputDirectory"]
    names = sorted(os.path.relpath(os.path.join(d, f), out) for d, _, fs in os.walk(out) for f in fs)
    want = sorted(["geometry_draco/%05d.drc" % k for k in range(5)] + ["texture_ktx2_baseColor_default/%05d.ktx2" % s for s in range(2)] +
                  ["texture_etc2_baseColor_default/%05d.etc2" % k for k in range(5)] + ["uvol.json"])
    assert names == want
    return open(os.path.join(out, "uvol.json"), "rb").read()
