"""TEST INFRASTRUCTURE: NumPy float32 restatement of the augmented upload (bod_upload_frames_u8_augmented) and of the ground-truth
map that goes with it (bod_augment_boxes), built on oracle/preprocess.py.  Shared by tests/test_gpu_augment.py and
tests/test_augment_host.py; nothing here calls the code under test."""
import math

import numpy as np

from oracle import preprocess as pp

IDENTITY = {"flip": 0, "scale": 1.0, "off_y": 0.5, "off_x": 0.5, "gain": 1.0, "bias": 0.0}


def record(**kw):
    out = dict(IDENTITY)
    out.update(kw)
    return out


def geometry(src_hw, net_hw, aspect_resize, scale=1.0, off_y=0.5, off_x=0.5):
    """(rh, rw, crop_y, crop_x, pad_y, pad_x) of one frame: the resize target grows by ``scale`` (float32, widened to double), the
    crop or pad of an axis is floor(off * |d|) of the size difference d (off float32, widened to double)."""
    sh, sw = int(src_hw[0]), int(src_hw[1])
    h, w = int(net_hw[0]), int(net_hw[1])
    s = float(np.float32(scale))

    def scaled(n):
        return max(1, int(math.floor(s * n + 0.5)))
    if aspect_resize:
        rh, rw = pp.preserve_aspect_size((sh, sw), (scaled(h), scaled(w)))
    else:
        assert (sh, sw) == (h, w)
        rh, rw = scaled(sh), scaled(sw)

    def place(d, off):
        o = float(np.float32(off))
        return (int(math.floor(o * d)) if d > 0 else 0), (int(math.floor(o * -d)) if d < 0 else 0)
    (cy, py), (cx, px) = place(rh - h, off_y), place(rw - w, off_x)
    return rh, rw, cy, cx, py, px


def augmented_frame(rgb_u8, net_hw, means, aspect_resize, rec):
    """One frame as the augmented upload must leave it: [H,W,3] float32 BGR, mean-subtracted."""
    h, w = int(net_hw[0]), int(net_hw[1])
    sh, sw = rgb_u8.shape[:2]
    rh, rw, cy, cx, py, px = geometry((sh, sw), net_hw, aspect_resize, rec["scale"], rec["off_y"], rec["off_x"])
    src = rgb_u8[:, ::-1] if rec["flip"] else rgb_u8                   # the flip acts on the source frame
    if aspect_resize or (rh, rw) != (sh, sw):
        x = pp.bilinear_resize(src, rh, rw)
    else:
        x = np.asarray(src, np.float32)
    vh, vw = min(rh, h), min(rw, w)
    vis = x[cy:cy + vh, cx:cx + vw]
    t = np.float32(rec["gain"]) * vis                                   # two separate float32 operations
    t = t + np.float32(rec["bias"])
    vis = np.minimum(np.maximum(t, np.float32(0)), np.float32(255))
    out = np.zeros((h, w, 3), np.float32)                               # padding stays 0 (-> -mean)
    out[py:py + vh, px:px + vw] = vis
    return pp.normalize_bgr(out, means)


def augmented_boxes(src_hw, net_hw, aspect_resize, rec, boxes, classes, min_visible):
    """Ground truth (y1,x1,y2,x2) in source pixels -> the augmented frame's network pixels, float32 throughout."""
    f = np.float32
    sh, sw = int(src_hw[0]), int(src_hw[1])
    h, w = int(net_hw[0]), int(net_hw[1])
    rh, rw, cy, cx, py, px = geometry(src_hw, net_hw, aspect_resize, rec["scale"], rec["off_y"], rec["off_x"])
    b = np.asarray(boxes, f).reshape(-1, 4).copy()
    c = np.asarray(classes, f).reshape(b.shape[0], -1)
    if rec["flip"]:
        x1 = f(sw - 1) - b[:, 3]
        x2 = f(sw - 1) - b[:, 1]
        b[:, 1], b[:, 3] = x1, x2
    ky, kx = f(rh / sh), f(rw / sw)
    t = b * np.asarray([ky, kx, ky, kx], f)
    t = t + np.asarray([py - cy, px - cx, py - cy, px - cx], f)
    lim = np.asarray([h - 1, w - 1, h - 1, w - 1], f)
    cl = np.minimum(np.maximum(t, f(0)), lim)
    ch, cw = cl[:, 2] - cl[:, 0], cl[:, 3] - cl[:, 1]
    full = (t[:, 2] - t[:, 0]) * (t[:, 3] - t[:, 1])
    keep = (ch >= 1) & (cw >= 1) & ~(ch * cw < f(min_visible) * full)
    if not keep.any():
        bg = np.zeros((1, c.shape[1]), f)
        bg[0, -1] = 1
        return np.asarray([[0, 0, 1, 1]], f), bg
    return cl[keep], c[keep]
