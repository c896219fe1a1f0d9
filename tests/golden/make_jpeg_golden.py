"""Writes tests/golden/jpeg_cases.npz: small JPEG files made by PIL with PIL's own decode of each, the corpus of the JPEG decoder's
tests.  Run once, by hand: `python tests/golden/make_jpeg_golden.py`.  PIL only: the GPU tests then do not depend
on the PIL / libjpeg build of the machine they run on.

Cases: sizes x content x sampling x quality x variant, thinned to six cases per (size, sampling) pair -- every pair stays, and the
24 (content, quality, variant) combinations rotate through the pairs so each appears twelve times.  The shapes are the smallest at
which the decoder can still go wrong: edge replication, chroma width <= 2, partial MCUs, restart resets, custom Huffman tables,
saturation.  Plus one progressive file, one CMYK file and one PNG as inputs the decoder must refuse."""
import io
import os

import numpy as np
from PIL import Image

SIZES = [(1, 1), (2, 1), (1, 3), (3, 3), (5, 4), (8, 8), (17, 2), (2, 17), (16, 16), (33, 47), (31, 5), (64, 48)]      # (w, h)
SAMPLINGS = ["4:4:4", "4:2:2", "4:2:0", "gray"]
CONTENTS = ["noise", "smooth"]
QUALITIES = [1, 30, 90, 100]
VARIANTS = ["plain", "restart", "optimize"]
PER_PAIR = 6


def make_image(w, h, content, gray, seed):
    rng = np.random.default_rng(seed)
    if content == "noise":
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    else:
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
        a = np.stack([255.0 * xx / max(w - 1, 1), 255.0 * yy / max(h - 1, 1), 255.0 - 127.0 * (xx + yy) / max(w + h - 2, 1)], axis=2)
        a = np.clip(a + rng.normal(0.0, 2.0, a.shape), 0, 255).astype(np.uint8)
    return Image.fromarray(a[:, :, 0], "L") if gray else Image.fromarray(a, "RGB")


def encode(im, sampling, quality, variant):
    kw = {"quality": quality}
    if sampling != "gray":
        kw["subsampling"] = sampling
    if variant == "restart":
        kw["restart_marker_blocks"] = 1
    elif variant == "optimize":
        kw["optimize"] = True
    buf = io.BytesIO()
    im.save(buf, "JPEG", **kw)
    return buf.getvalue()


def pil_rgb(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def main():
    files, rgbs, meta = [], [], []
    pair = 0
    for si, (w, h) in enumerate(SIZES):
        for pi, sampling in enumerate(SAMPLINGS):
            for k in range(PER_PAIR):
                combo = ((pair * PER_PAIR + k) * 7) % 24
                ci, qi, vi = combo % 2, (combo // 2) % 4, combo // 8
                im = make_image(w, h, CONTENTS[ci], sampling == "gray", seed=1000 * pair + k)
                data = encode(im, sampling, QUALITIES[qi], VARIANTS[vi])
                rgb = pil_rgb(data)
                assert rgb.shape == (h, w, 3)
                files.append(data)
                rgbs.append(rgb)
                meta.append((w, h, pi, ci, QUALITIES[qi], vi))
            pair += 1
    base = make_image(24, 16, "smooth", False, seed=7)
    buf = io.BytesIO(); base.save(buf, "JPEG", quality=80, progressive=True); progressive = buf.getvalue()
    buf = io.BytesIO(); base.convert("CMYK").save(buf, "JPEG", quality=80); cmyk = buf.getvalue()
    buf = io.BytesIO(); base.save(buf, "PNG"); png = buf.getvalue()
    out = {
        "jpeg_bytes": np.frombuffer(b"".join(files), np.uint8),
        "jpeg_offsets": np.cumsum([0] + [len(f) for f in files]).astype(np.int64),
        "rgb_bytes": np.concatenate([r.reshape(-1) for r in rgbs]),
        "meta": np.array(meta, np.int32),                 # width, height, sampling, content, quality, variant (indices into the lists above)
        "progressive": np.frombuffer(progressive, np.uint8), "progressive_rgb": pil_rgb(progressive),
        "cmyk": np.frombuffer(cmyk, np.uint8),
        "png": np.frombuffer(png, np.uint8), "png_rgb": pil_rgb(png),
    }
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "jpeg_cases.npz")
    np.savez_compressed(path, **out)
    print("%d cases, %d file bytes, %d RGB bytes -> %s (%d bytes)" % (len(files), len(out["jpeg_bytes"]), len(out["rgb_bytes"]), path,
                                                                    os.path.getsize(path)))


if __name__ == "__main__":
    main()
