"""Detections and their corner uncertainty drawn onto frames on the GPU (the drawing contract: include/bayesod.h).

``render_frames`` is ``bod_render_frames_u8``: a batch of uint8 RGB frames of any sizes and, per frame, a ``Detections`` record (integer
corner boxes x0 y0 x1 y1, the two 2x2 corner covariances in (x, y) order, a colour and a label of up to 16 glyphs) -> the frames with

  * ``view='overlay'``: ground-truth rings, every detection's box and label, and a 2-sigma ellipse on its two corners;
  * ``view='heat'``: the jet-coloured spatial-probability map of PDQ's box heatmaps (``prob_detection_quality``), blended 0.9 / 0.1.

``detections_from_tree`` reads one frame of a prediction tree (``writers.PredictionWriter``: mean/ cov/ cat_param/) into that record.
"""
import collections
import ctypes as C
import os

import numpy as np

from . import _lib
from .prob_detection_quality import _VUHW_TO_CORNERS

R2_TWO_SIGMA = 6.180074                        # chi2.ppf(2 * Phi(2) - 1, 2): the contour that holds what +-2 sigma holds in 1-D
CHARSET = "abcdefghijklmnopqrstuvwxyz0123456789. %-_"
TEXT_LEN = 16
VIEWS = {'overlay': _lib.BOD_RENDER_OVERLAY, 'heat': _lib.BOD_RENDER_HEAT}
# one colour per class index (cycled): the defaults of the overlays
PALETTE = ((255, 64, 64), (64, 160, 255), (255, 208, 0), (200, 96, 255), (0, 224, 160), (255, 128, 0), (240, 240, 240), (255, 96, 192),
           (128, 224, 0), (96, 96, 255))

Detections = collections.namedtuple('Detections', 'boxes corner_covs colors text')
Detections.__doc__ = """One frame's rows: boxes int32 [D,4] x0 y0 x1 y1, corner_covs float32 [D,2,2,2] (top-left then bottom-right,
(x, y) order), colors uint8 [D,3] RGB, text uint8 [D,16] glyph indices (0xFF ends a label)."""


def font():
    """The label font as uint8 [41, 7, 5] (glyph, row, column) of 0 / 1, read from the library (csrc/render_font.h is the one copy)."""
    lib = _lib.load()
    count = C.c_int32(0)
    _lib.check(lib, None, lib.bod_render_font(None, C.byref(count)))
    rows = np.zeros((count.value, 7), np.uint8)
    _lib.check(lib, None, lib.bod_render_font(rows.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(count)))
    return ((rows[:, :, None] >> np.arange(4, -1, -1)) & 1).astype(np.uint8)


def encode_text(s):
    """A label as 16 glyph indices: lower-cased, characters outside the charset become '_', cut at 16, 0xFF after the end."""
    out = np.full(TEXT_LEN, 0xFF, np.uint8)
    for i, ch in enumerate(str(s).lower()[:TEXT_LEN]):
        k = CHARSET.find(ch)
        out[i] = k if k >= 0 else CHARSET.index('_')
    return out


def make_detections(boxes=None, corner_covs=None, colors=None, labels=None):
    """``Detections`` from array-likes; colours default to the palette's first, labels (strings) to none."""
    boxes = np.ascontiguousarray(np.asarray(boxes if boxes is not None else [], np.int32).reshape(-1, 4))
    d = len(boxes)
    covs = np.ascontiguousarray(np.asarray(corner_covs if corner_covs is not None else [], np.float32).reshape(-1, 2, 2, 2))
    if len(covs) != d:
        raise ValueError("%d boxes but %d corner covariances" % (d, len(covs)))
    if colors is None:
        colors = np.tile(np.asarray(PALETTE[0], np.uint8), (d, 1))
    colors = np.ascontiguousarray(np.asarray(colors, np.uint8).reshape(-1, 3))
    if len(colors) != d:
        raise ValueError("%d boxes but %d colours" % (d, len(colors)))
    text = np.full((d, TEXT_LEN), 0xFF, np.uint8)
    if labels is not None:
        if len(labels) != d:
            raise ValueError("%d boxes but %d labels" % (d, len(labels)))
        for i, s in enumerate(labels):
            text[i] = s if isinstance(s, np.ndarray) else encode_text(s)
    return Detections(boxes, covs, colors, text)


def render_options(view='overlay', line_width=2, labels=True, r2=R2_TWO_SIGMA):
    if view not in VIEWS:
        raise ValueError("view %r is not one of %s" % (view, sorted(VIEWS)))
    return _lib.BodRenderOptions(VIEWS[view], int(line_width), int(bool(labels)), float(r2), (C.c_int32 * 4)(0, 0, 0, 0))


def pack(frames, detections, gt_boxes=None):
    """The arrays of one ``bod_render_frames_u8`` call: (packed frames, src_hw, num_det, boxes, covs, colors, text, num_gt, gt)."""
    frames = [np.ascontiguousarray(f, np.uint8) for f in frames]
    for f in frames:
        if f.ndim != 3 or f.shape[2] != 3:
            raise ValueError("a frame is %s, not [h, w, 3]" % (f.shape,))
    if len(detections) != len(frames) or (gt_boxes is not None and len(gt_boxes) != len(frames)):
        raise ValueError("%d frames need as many detection (and ground-truth) records" % len(frames))
    detections = [d if isinstance(d, Detections) else make_detections(*d) for d in detections]
    buf = np.concatenate([f.reshape(-1) for f in frames]) if frames else np.zeros(0, np.uint8)
    src_hw = np.asarray([f.shape[:2] for f in frames], np.int32).reshape(-1, 2)
    num_det = np.asarray([len(d.boxes) for d in detections], np.int32)

    def cat(parts, shape, dtype):
        if not parts:
            return np.zeros((0,) + shape[1:], dtype)
        return np.ascontiguousarray(np.concatenate([np.asarray(p, dtype).reshape(shape) for p in parts]))
    boxes = cat([d.boxes for d in detections], (-1, 4), np.int32)
    covs = cat([d.corner_covs for d in detections], (-1, 2, 2, 2), np.float32)
    colors = cat([d.colors for d in detections], (-1, 3), np.uint8)
    text = cat([d.text for d in detections], (-1, TEXT_LEN), np.uint8)
    num_gt = gt = None
    if gt_boxes is not None:
        gts = [np.asarray(g, np.int32).reshape(-1, 4) for g in gt_boxes]
        num_gt = np.asarray([len(g) for g in gts], np.int32)
        gt = cat(gts, (-1, 4), np.int32)
    return buf, src_hw, num_det, boxes, covs, colors, text, num_gt, gt


def _u8ptr(a):
    return None if a is None or a.size == 0 else a.ctypes.data_as(C.POINTER(C.c_uint8))


def _ptr(a, conv):
    return None if a is None or a.size == 0 else conv(a)


def render_frames(frames, detections, view='overlay', line_width=2, labels=True, r2=R2_TWO_SIGMA, gt_boxes=None, device=0,
                  return_skipped=False):
    """Draws every frame's detections in ONE ``bod_render_frames_u8`` call (frames of mixed sizes share it) and returns the list of
    rendered uint8 [h, w, 3] frames; with ``return_skipped`` also the int32 [n] count of ellipses skipped per frame (a corner
    covariance that is not finite and positive definite in float32).  ``gt_boxes``: per frame int [G, 4] x0 y0 x1 y1, drawn green."""
    lib = _lib.load()
    buf, src_hw, num_det, boxes, covs, colors, text, num_gt, gt = pack(frames, detections, gt_boxes)
    n = len(src_hw)
    out = np.empty_like(buf)
    skipped = np.zeros(n, np.int32)
    opt = render_options(view, line_width, labels, r2)
    st = lib.bod_render_frames_u8(int(device), n, _u8ptr(buf), _ptr(src_hw, _lib.iptr), _lib.iptr(num_det) if n else None,
                                  _ptr(boxes, _lib.iptr), _ptr(covs, _lib.fptr), _u8ptr(colors), _u8ptr(text),
                                  _lib.iptr(num_gt) if num_gt is not None and n else None, _ptr(gt, _lib.iptr), C.byref(opt), _u8ptr(out),
                                  _lib.iptr(skipped) if n else None)
    _lib.check(lib, None, st)
    res, off = [], 0
    for h, w in src_hw:
        res.append(out[off:off + 3 * h * w].reshape(h, w, 3))
        off += 3 * h * w
    return (res, skipped) if return_skipped else res


def corner_covariances(covs_vuhw, cov_scale=1.0):
    """[K,4,4] covariances of (v, u, h, w) -> float64 [K,2,2,2]: the covariance of the top-left and of the bottom-right corner in
    (x, y) order, from Sigma_corners = T Sigma T^T with T the map (v, u, h, w) -> (u1, v1, u2, v2) = (x0, y0, x1, y1)."""
    s = np.asarray(covs_vuhw, np.float64).reshape(-1, 4, 4) * float(cov_scale)
    c = np.matmul(np.matmul(_VUHW_TO_CORNERS, s), _VUHW_TO_CORNERS.T)
    return np.stack([c[:, 0:2, 0:2], c[:, 2:4, 2:4]], axis=1)


def detections_from_tree(tree, frame, min_score=0.5, cov_scale=1.0, categories=None, palette=None, cov_dir='cov'):
    """One frame of a prediction tree as ``Detections``: rows of ``mean/<frame>.npy`` (v, u, h, w) whose best class score in
    ``cat_param/<frame>.npy`` reaches ``min_score``; corners truncated to integers, corner covariances from ``<cov_dir>/<frame>.npy``
    (``cov_epistemic`` etc. of a --covariance_parts tree work the same) times ``cov_scale``, colour = palette[class], label
    "<name> <score:.2f>" with the class's name from ``categories`` (its index without)."""
    palette = PALETTE if palette is None else palette
    mean = np.asarray(np.load(os.path.join(tree, 'mean', frame + '.npy')), np.float64).reshape(-1, 4)
    cov = np.asarray(np.load(os.path.join(tree, cov_dir, frame + '.npy')), np.float64).reshape(-1, 4, 4)
    cat = np.asarray(np.load(os.path.join(tree, 'cat_param', frame + '.npy')), np.float64)
    cat = cat.reshape(len(mean), -1) if len(mean) else np.zeros((0, 1))
    if len(cov) != len(mean):
        raise ValueError("%s: %d means but %d covariances in %s/" % (frame, len(mean), len(cov), cov_dir))
    cls = cat.argmax(axis=1) if len(mean) else np.zeros(0, np.int64)
    score = cat.max(axis=1) if len(mean) else np.zeros(0)
    keep = score >= min_score
    v, u, h, w = mean[keep].T
    boxes = np.stack([u - w / 2.0, v - h / 2.0, u + w / 2.0, v + h / 2.0], axis=1)
    boxes = np.clip(boxes, -2.0 ** 30, 2.0 ** 30).astype(np.int32)
    labels = []
    for k, s in zip(cls[keep], score[keep]):
        name = categories[k] if categories is not None and k < len(categories) else str(int(k))
        labels.append("%s %.2f" % (name, s))
    colors = np.asarray([palette[int(k) % len(palette)] for k in cls[keep]], np.uint8).reshape(-1, 3)
    return make_detections(boxes, corner_covariances(cov[keep], cov_scale).astype(np.float32), colors, labels)
