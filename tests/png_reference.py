"""NumPy restatement of the PNG scanline filters' reconstruction (PNG specification, section 9) and of the colour types' way to RGB:
what png_unfilter_kernel computes, written independently of it.  tests/test_png_host.py holds it against PIL on the
corpus; the GPU tests' failure messages compare against it."""
import numpy as np


def unfilter(raw, bpp):
    """raw uint8 [h, 1 + n] (filter-type byte, then n = width * bpp filtered bytes per row) -> the reconstructed bytes uint8 [h, n]."""
    raw = np.asarray(raw)
    h, n = raw.shape[0], raw.shape[1] - 1
    out = np.zeros((h, n), np.int64)
    prev = np.zeros(n, np.int64)
    for r in range(h):
        ft, f = int(raw[r, 0]), raw[r, 1:].astype(np.int64)
        if ft == 0:
            row = f.copy()
        elif ft == 2:
            row = (f + prev) & 255
        elif ft == 1:
            row = f.copy()
            for lane in range(bpp):                                   # a running sum per byte lane
                row[lane::bpp] = np.cumsum(f[lane::bpp]) & 255
        elif ft in (3, 4):
            row = np.zeros(n, np.int64)
            for i in range(n):
                a = row[i - bpp] if i >= bpp else 0
                b = prev[i]
                c = prev[i - bpp] if i >= bpp else 0
                if ft == 3:
                    pred = (a + b) >> 1
                else:
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
                row[i] = (f[i] + pred) & 255
        else:
            raise ValueError("filter type %d in row %d" % (ft, r))
        out[r] = row
        prev = row
    return out.astype(np.uint8)


def to_rgb(recon, width, channels):
    """Reconstructed bytes [h, width * channels] -> uint8 [h, width, 3]: RGB, RGBA without alpha, gray (+ alpha) three times."""
    px = recon.reshape(recon.shape[0], width, channels)
    if channels >= 3:
        return np.ascontiguousarray(px[:, :, :3])
    return np.ascontiguousarray(np.repeat(px[:, :, :1], 3, axis=2))


def decode(raw, width, channels):
    return to_rgb(unfilter(raw, channels), width, channels)
