"""Loader of tests/golden/jpeg_cases.npz (written by tests/golden/make_jpeg_golden.py): the JPEG decoder tests' corpus."""
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_cases.npz")
SAMPLINGS = ["4:4:4", "4:2:2", "4:2:0", "gray"]
LUMA = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2), "gray": (1, 1)}
VARIANTS = ["plain", "restart", "optimize"]
_cache = {}


class Case:
    def __init__(self, index, data, rgb, meta):
        self.index, self.data, self.rgb = index, data, rgb
        self.width, self.height = int(meta[0]), int(meta[1])
        self.sampling, self.content, self.quality = SAMPLINGS[meta[2]], ("noise", "smooth")[meta[3]], int(meta[4])
        self.variant = VARIANTS[meta[5]]

    def __repr__(self):
        return "case %d: %dx%d %s %s q%d %s" % (self.index, self.width, self.height, self.sampling, self.content, self.quality, self.variant)


def load():
    """-> (cases, extras): the supported cases, and the byte strings / PIL decodes of the progressive, CMYK and PNG files."""
    if "v" not in _cache:
        z = np.load(PATH)
        off, meta = z["jpeg_offsets"], z["meta"]
        blob, rgb = z["jpeg_bytes"].tobytes(), z["rgb_bytes"]
        cases, r = [], 0
        for i in range(len(meta)):
            w, h = int(meta[i, 0]), int(meta[i, 1])
            a = rgb[r:r + 3 * w * h].reshape(h, w, 3)
            a.setflags(write=False)
            cases.append(Case(i, blob[off[i]:off[i + 1]], a, meta[i]))
            r += 3 * w * h
        extras = {"progressive": z["progressive"].tobytes(), "progressive_rgb": z["progressive_rgb"], "cmyk": z["cmyk"].tobytes(),
                  "png": z["png"].tobytes(), "png_rgb": z["png_rgb"]}
        _cache["v"] = (cases, extras)
    return _cache["v"]
