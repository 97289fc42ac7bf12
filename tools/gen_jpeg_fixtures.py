#!/usr/bin/env python3
"""Writes tests/golden/jpeg/: the small JPEG files the JPEG tests read (tests/jpeg_cases.py), and expected.npz with Pillow's (libjpeg-turbo's)
own decode of every accepted file - the tests then need neither Pillow nor this tool.  Needs Pillow and NumPy; run it from anywhere:

    python3 tools/gen_jpeg_fixtures.py

The set is the smallest shapes at which the decoder can still go wrong: 1 x 1 and 8 x 8 grey; 16 x 16 at 4:2:0 (one MCU: every neighbour is an
edge); 17 x 9 and 47 x 17 at 4:2:0 (partial MCUs on both axes, odd chroma extents); 24 x 40 at 4:2:2 (the real extent ends inside a block);
33 x 31 at 4:4:4; qualities 1 (table entries up to 255) and 100 (all ones); optimised Huffman tables; restart markers per block and per row; a
file whose entropy data holds a stuffed FF 00 (checked here); a five-frame 24 x 24 4:2:0 sequence with a quality per frame; and the refusals:
progressive, CMYK, a 4:4:4 file patched to declare luma 1 x 2, a file truncated in its scan, a file without its DHT segments."""
import io
import os
import numpy as np
from PIL import Image

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "jpeg")


def picture(w, h, seed, kind="mix"):
    """smooth ramps, a hard-edged rectangle and some noise, in colour"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    a = np.empty((h, w, 3), np.float64)
    a[..., 0] = 40 + 170 * x / max(w - 1, 1)
    a[..., 1] = 220 - 180 * y / max(h - 1, 1)
    a[..., 2] = 128 + 100 * np.sin(x / 3.0 + y / 5.0)
    if kind != "smooth":
        a[h // 4:h // 4 + max(h // 3, 1), w // 3:w // 3 + max(w // 3, 1)] = (250, 10, 240)
        a += rng.normal(0, 60 if kind == "noise" else 12, a.shape)
    return np.clip(a, 0, 255).astype(np.uint8)


def jpeg(arr, mode="RGB", **kw):
    if mode == "L":
        im = Image.fromarray(arr[..., 1])
    elif mode == "CMYK":
        im = Image.fromarray(np.ascontiguousarray(np.dstack([arr, arr[..., :1]])), "CMYK")
    else:
        im = Image.fromarray(arr)
    b = io.BytesIO(); im.save(b, "JPEG", **kw); return b.getvalue()


def segments(data):
    """[(marker, start, end)] of the segments ahead of the scan, and the offset of the entropy data"""
    out = []; p = 2
    while True:
        assert data[p] == 0xFF
        m = data[p + 1]; L = (data[p + 2] << 8) | data[p + 3]
        out.append((m, p, p + 2 + L)); p += 2 + L
        if m == 0xDA:
            return out, p


def main():
    os.makedirs(OUT, exist_ok=True)
    files = {
        "grey_1x1": jpeg(picture(1, 1, 1), "L", quality=90),
        "grey_8x8": jpeg(picture(8, 8, 2), "L", quality=85),
        "c420_16x16": jpeg(picture(16, 16, 3), quality=90, subsampling=2),
        "c420_17x9": jpeg(picture(17, 9, 4), quality=92, subsampling=2),
        "c420_47x17": jpeg(picture(47, 17, 5), quality=80, subsampling=2),
        "c422_24x40": jpeg(picture(24, 40, 6), quality=88, subsampling=1),
        "c444_33x31": jpeg(picture(33, 31, 7), quality=75, subsampling=0),
        "q1_420_19x13": jpeg(picture(19, 13, 8, "noise"), quality=1, subsampling=2),
        "q100_444_20x12": jpeg(picture(20, 12, 9, "noise"), quality=100, subsampling=0),
        "opt_420_24x24": jpeg(picture(24, 24, 10), quality=85, subsampling=2, optimize=True),
        "rstblk_420_33x17": jpeg(picture(33, 17, 11), quality=85, subsampling=2, restart_marker_blocks=1),
        "rstrow_422_40x20": jpeg(picture(40, 20, 12), quality=85, subsampling=1, restart_marker_rows=1),
        "stuffed_444_24x16": jpeg(picture(24, 16, 13, "noise"), quality=98, subsampling=0),
    }
    for k, q in enumerate((35, 60, 75, 90, 97)):
        files["seq_%d" % k] = jpeg(picture(24, 24, 20 + k), quality=q, subsampling=2)
    # the stuffed byte is in the entropy data, and the restart files do hold RSTn markers
    segs, scan = segments(files["stuffed_444_24x16"])
    assert b"\xff\x00" in files["stuffed_444_24x16"][scan:], "no stuffed FF 00: change the seed"
    for name in ("rstblk_420_33x17", "rstrow_422_40x20"):
        assert any(m == 0xDD for m, _, _ in segments(files[name])[0]) and b"\xff\xd0" in files[name], name
    dht = lambda data: b"".join(data[a:b] for m, a, b in segments(data)[0] if m == 0xC4)
    assert dht(files["opt_420_24x24"]) != dht(files["seq_0"]), "the optimised file carries the default tables"
    expected = {}
    for name, data in files.items():
        expected[name] = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
    # the refusals
    base = files["c444_33x31"]
    segs, scan = segments(base)
    sof = [s for s in segs if s[0] == 0xC0][0]
    patched = bytearray(base); assert patched[sof[1] + 11] == 0x11; patched[sof[1] + 11] = 0x12      # component 0: H = 1, V = 2
    nodht = bytearray(base)
    for m, a, b in reversed(segs):
        if m == 0xC4:
            del nodht[a:b]
    refused = {
        "bad_progressive": jpeg(picture(24, 24, 30), quality=85, progressive=True),
        "bad_cmyk": jpeg(picture(16, 16, 31), "CMYK", quality=85),
        "bad_luma_1x2": bytes(patched),
        "bad_truncated": base[:scan + (len(base) - scan) // 2],
        "bad_no_dht": bytes(nodht),
    }
    for name, data in list(files.items()) + list(refused.items()):
        assert len(data) < 8192, (name, len(data))
        with open(os.path.join(OUT, name + ".jpg"), "wb") as f:
            f.write(data)
    np.savez_compressed(os.path.join(OUT, "expected.npz"), **expected)
    print("%d files, %d bytes; expected.npz %d bytes" % (len(files) + len(refused), sum(map(len, files.values())) + sum(map(len, refused.values())),
                                                        os.path.getsize(os.path.join(OUT, "expected.npz"))))


if __name__ == "__main__":
    main()
