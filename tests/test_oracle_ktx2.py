"""CPU oracle vs the reference's .ktx2 fixtures + oracle ETC1S encoder round trips."""
import json
import os
import struct
import numpy as np
import pytest
from conftest import GOLDEN, REF_OUT

GOLD = json.load(open(os.path.join(GOLDEN, "ktx2_goldens.json")))
TEXDIR = os.path.join(REF_OUT, "texture_ktx2-fps30-1k_baseColor_default")


def test_survey_appendix_values():
    f0 = GOLD["files"]["00000.ktx2"]
    assert (f0["size"], f0["width"], f0["height"], f0["layers"], f0["supercomp"], f0["dfd_model"]) == (232441, 1024, 1024, 5, 1, 163)
    assert (f0["sgd_off"], f0["sgd_len"], f0["level_off"], f0["level_len"]) == (216, 5422, 5638, 226803)
    assert (f0["n_endpoints"], f0["n_selectors"], f0["endpoints_len"], f0["selectors_len"], f0["tables_len"], f0["hist_size"]) == (1506, 734, 2789, 1598, 915, 64)
    assert (f0["ep_bits"], f0["sel_bits"], f0["tab_bits"]) == (22309, 12780, 7318)
    assert f0["slice_flags"] == [0, 2, 2, 2, 2] and f0["slice_len"] == [81805, 37466, 36123, 35947, 35462]
    assert f0["slice_bits"] == [654434, 299722, 288981, 287570, 283690] and f0["slice_skip"] == [0, 43794, 44830, 44968, 45073]
    assert f0["first_endpoints"] == [[0, 0, 0, 0], [10, 10, 9, 6], [19, 15, 14, 0]] and f0["writer"] == "Basis Universal 1.16"
    fs = GOLD["files"]
    assert GOLD["n_files"] == 50 and sum(sum(v["slice_skip"]) for v in fs.values()) == 8984009
    assert (min(v["n_endpoints"] for v in fs.values()), max(v["n_endpoints"] for v in fs.values())) == (1489, 1532)
    assert (min(v["n_selectors"] for v in fs.values()), max(v["n_selectors"] for v in fs.values())) == (728, 744)
    assert all(v["slice_flags"] == [0, 2, 2, 2, 2] for v in fs.values())
    assert max(8 * l - b for v in fs.values() for l, b in zip(v["slice_len"], v["slice_bits"])) <= 7


def test_decoder_on_committed_fixture(oracle):
    g = oracle.ktx2_goldens(open(os.path.join(GOLDEN, "00000.ktx2"), "rb").read())
    assert g == GOLD["files"]["00000.ktx2"]


def test_decoder_on_all_50_reference_fixtures(oracle):
    for name, g in sorted(GOLD["files"].items()):
        assert oracle.ktx2_goldens(open(os.path.join(TEXDIR, name), "rb").read()) == g, name


def _check_container(k, w, h, layers):
    """Header / DFD / KVD layout per SURVEY B.0 (what src/lib/KTX2Loader.js:297-301 and ktx-parse read)."""
    assert k[:12] == bytes([0xAB]) + b"KTX 20" + bytes([0xBB]) + b"\r\n\x1a\n"
    vk, ts, pw, ph, pd, lc, fc, lv, sc = struct.unpack_from("<9I", k, 12)
    assert (vk, ts, pw, ph, pd, lc, fc, lv, sc) == (0, 1, w, h, 0, layers, 1, 1, 1)
    dfd_off, dfd_len, kvd_off, kvd_len = struct.unpack_from("<4I", k, 48)
    sgd_off, sgd_len, lvl_off, lvl_len, lvl_ulen = struct.unpack_from("<5Q", k, 64)
    assert (dfd_off, dfd_len, kvd_off) == (104, 44, 148) and sgd_off % 8 == 0 and lvl_off == sgd_off + sgd_len and lvl_off + lvl_len == len(k) and lvl_ulen == 0
    ref_dfd = bytes.fromhex("2c000000" "00000000" "02002800" "a3010200" "03030000" "0000000000000000" "00003f00" "00000000" "00000000" "ffffffff")
    assert k[104:148] == ref_dfd
    assert k[152:164] == b"KTXanimData\0" and struct.unpack_from("<3I", k, 164) == (1, 15, 0)
    assert lc >= 2 or layers == 1      # the stock player needs an array texture


@pytest.mark.parametrize("size,n,seed", [(64, 2, 1), (128, 3, 2), (100, 2, 3)])
def test_encoder_roundtrip(oracle, size, n, seed):
    import synth
    tex = synth.texture_sequence(n, size=size, seed=seed)
    k = oracle.ktx2_encode(tex)
    _check_container(k, size, size, n)
    d = oracle.ktx2_decode(k)
    assert d.slice_flags == [0] + [2] * (n - 1) and d.hist_size == 64
    assert all(8 * l - b <= 7 for l, b in zip(d.slice_len, d.slice_bits_used))
    assert d.slice_skip[0] == 0 and all(s > 0 for s in d.slice_skip[1:])
    for l in range(n):
        assert oracle.psnr(d.images[l], tex[l][::-1]) > 30.0      # stored rows are bottom-up (-y_flip)


def test_encoder_on_reference_texture(oracle):
    """Real captured content: re-encode the decoded reference segment; bpp and codebook sizes land at the
    fixture's operating point (Basis Universal 1.16 defaults: 0.355 bpp, 1506/734 entries)."""
    ref = open(os.path.join(GOLDEN, "00000.ktx2"), "rb").read()
    d = oracle.ktx2_decode(ref)
    src = [im[::-1].copy() for im in d.images]
    k = oracle.ktx2_encode(src)
    e = oracle.ktx2_decode(k)
    assert 0.8 * len(ref) < len(k) < 1.1 * len(ref)
    assert 1200 <= e.n_endpoints <= 1536 and 600 <= e.n_selectors <= 768
    assert min(oracle.psnr(e.images[l], d.images[l]) for l in range(5)) > 38.0
    assert all(40000 < s < 60000 for s in e.slice_skip[1:])


def test_encoder_flat_and_single_layer(oracle):
    flat = [np.full((16, 16, 4), 255, np.uint8)]
    flat[0][..., :3] = (12, 200, 77)
    k = oracle.ktx2_encode(flat)
    d = oracle.ktx2_decode(k)
    assert d.n_endpoints == 1 and d.n_selectors == 1
    assert np.abs(d.images[0][..., :3].astype(int) - flat[0][..., :3].astype(int)).max() <= 8


@pytest.mark.skipif(not os.path.exists("/root/reference/src/lib/ktx-parse.module.js"), reason="/root/reference only exists in the build container")
def test_container_cross_read_with_the_reference_ktx_parse(oracle, tmp_path):
    """SURVEY 8(c) 'other in-repo oracles': the reference's own vendored KTX-Parse (src/lib/ktx-parse.module.js, what the stock
    KTX2Loader uses for the container, KTX2Loader.js:299-301) reads this encoder's ETC1S file and the reference's fixture to the same
    header / DFD / key-value fields.  A third-party reader, not the builder's decoder; needs node >= 12 (part of this container)."""
    import shutil, subprocess, synth
    node = shutil.which("node")
    assert node, "node (>= 12) is part of this container: the cross-read must run, not be skipped"
    shutil.copy("/root/reference/src/lib/ktx-parse.module.js", tmp_path / "ktxparse.mjs")
    mine = oracle.ktx2_encode(synth.texture_sequence(3, size=64, seed=1))
    (tmp_path / "mine.ktx2").write_bytes(mine)
    shutil.copy(os.path.join(GOLDEN, "00000.ktx2"), tmp_path / "ref.ktx2")
    js = ("import { read } from './ktxparse.mjs'; import fs from 'fs';"
          "const out = {};"
          "for (const n of ['mine', 'ref']) { const c = read(new Uint8Array(fs.readFileSync(n + '.ktx2'))); const d = c.dataFormatDescriptor[0];"
          " out[n] = {vk: c.vkFormat, ts: c.typeSize, w: c.pixelWidth, h: c.pixelHeight, d: c.pixelDepth, layers: c.layerCount, faces: c.faceCount, sc: c.supercompressionScheme,"
          " model: d.colorModel, prim: d.colorPrimaries, transfer: d.transferFunction, flags: d.flags, dim: Array.from(d.texelBlockDimension), samples: d.samples.length,"
          " bitLength: d.samples[0].bitLength, chan: d.samples[0].channelID === undefined ? d.samples[0].channelType : d.samples[0].channelID,"
          " kv: Object.keys(c.keyValue).sort(), levels: c.levels.length, ep: c.globalData.endpointCount, sel: c.globalData.selectorCount, images: c.globalData.imageDescs.length}; }"
          "console.log(JSON.stringify(out))")
    (tmp_path / "r.mjs").write_text(js)
    r = subprocess.run([node, "--experimental-modules", "r.mjs"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-800:]
    o = json.loads(r.stdout.strip().splitlines()[-1])
    d = oracle.ktx2_decode(mine)
    same = ("vk", "ts", "d", "faces", "sc", "model", "prim", "transfer", "flags", "dim", "samples", "bitLength", "chan", "levels")
    assert {k: o["mine"][k] for k in same} == {k: o["ref"][k] for k in same}          # same container family as `basisu -ktx2 -tex_type video`
    assert (o["mine"]["w"], o["mine"]["h"], o["mine"]["layers"], o["mine"]["ep"], o["mine"]["sel"]) == (64, 64, 3, d.n_endpoints, d.n_selectors)
    assert (o["ref"]["w"], o["ref"]["layers"], o["ref"]["ep"], o["ref"]["sel"]) == (1024, 5, 1506, 734)
    assert "KTXanimData" in o["mine"]["kv"] and "KTXwriter" in o["mine"]["kv"] and o["mine"]["kv"] == o["ref"]["kv"]
    # a file with alpha slices: the reference's parser must see the second DFD sample (channel 15, bit 64) and the image descs' second
    # offset / length pair where this encoder put them
    from test_hipemu_tex import _alpha_sequence
    alpha = oracle.ktx2_encode(_alpha_sequence(2, 48, 3))
    (tmp_path / "alpha.ktx2").write_bytes(alpha)
    js2 = ("import { read } from './ktxparse.mjs'; import fs from 'fs';"
           "const c = read(new Uint8Array(fs.readFileSync('alpha.ktx2'))); const d = c.dataFormatDescriptor[0];"
           "const ch = s => s.channelID === undefined ? s.channelType : s.channelID;"
           "console.log(JSON.stringify({samples: d.samples.length, chan: d.samples.map(ch), off: d.samples.map(s => s.bitOffset), len: d.samples.map(s => s.bitLength), layers: c.layerCount,"
           " images: c.globalData.imageDescs.map(i => [i.imageFlags, i.rgbSliceByteOffset, i.rgbSliceByteLength, i.alphaSliceByteOffset, i.alphaSliceByteLength])}))")
    (tmp_path / "r2.mjs").write_text(js2)
    r = subprocess.run([node, "--experimental-modules", "r2.mjs"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-800:]
    a = json.loads(r.stdout.strip().splitlines()[-1]); da = oracle.ktx2_decode(alpha)
    assert a["samples"] == 2 and a["chan"] == [0, 15] and a["off"] == [0, 64] and a["len"] == [63, 63] and a["layers"] == 2 and da.has_alpha == 1
    # (this KTX-Parse reads one image desc per mip level, not per layer: the first image's is what can be compared)
    assert a["images"][0] == [da.slice_flags[0], da.slice_off[0], da.slice_len[0], da.slice_off[1], da.slice_len[1]]
    assert a["images"][0][0] == 0 and a["images"][0][3] == a["images"][0][2] and a["images"][0][4] > 0


def test_alpha_slices_round_trip(oracle):
    """VERDICT r2 #10 (parity with basisu unpinned: no reference file has alpha): an image with alpha != 255 gives every layer a second
    slice; colour and alpha come back through the decoder, the skip chain of the alpha slices is their own (a still alpha channel
    under changing colours skips every alpha block of the P-frames), opaque input is byte-identical to what it always was."""
    import synth
    from test_hipemu_tex import _alpha_sequence
    tex = _alpha_sequence(3, 64, 7)
    d = oracle.ktx2_decode(oracle.ktx2_encode(tex))
    assert d.has_alpha == 1 and d.layers == 3 and d.n_slices == 6 and d.slice_flags == [0, 0, 2, 2, 2, 2]
    for l in range(3):
        src = tex[l][::-1].astype(int); err = d.images[l].astype(int) - src
        assert (err[..., :3] ** 2).mean() < 150.0 and (err[..., 3] ** 2).mean() < 40.0
    still = [t.copy() for t in tex]
    for t in still: t[..., 3] = tex[0][..., 3]
    ds = oracle.ktx2_decode(oracle.ktx2_encode(still))
    nb = ds.bx * ds.by
    assert ds.slice_skip[3] == nb and ds.slice_skip[5] == nb and ds.slice_skip[2] < nb
    for l in range(3): assert np.array_equal(ds.images[l][..., 3], ds.images[0][..., 3])
    opaque = synth.texture_sequence(3, size=64, seed=7)
    do = oracle.ktx2_decode(oracle.ktx2_encode(opaque))
    assert do.has_alpha == 0 and do.n_slices == 3 and all((im[..., 3] == 255).all() for im in do.images)
