"""CPU: the rendering stage without a device -- the NumPy restatement of the drawing contract
(tests/render_reference.py) pinned by properties, the font through bod_render_font, ``render.detections_from_tree`` against a
hand-computed T Sigma T^T, and bod_render_frames_u8's argument validation (it runs before a device is looked for)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import conftest  # noqa: F401
import render_reference as ref

R2 = 6.180074


def _alpha_sum(a):
    return float(a.sum()) / 256.0


def test_ring_pixel_counts_and_widths():
    for (bw, bh) in [(2, 2), (5, 3), (17, 9)]:
        box = (10, 12, 10 + bw - 1, 12 + bh - 1)
        assert (ref.ring_alpha(48, 64, box, 1) == 256).sum() == 2 * (bw + bh) - 4
    a1 = ref.ring_alpha(1, 1, (0, 0, 0, 0), 1)
    assert a1[0, 0] == 256                                                     # a one-pixel box is its own ring
    box = (10, 12, 30, 25)
    ys, xs = np.mgrid[0:48, 0:64]
    # width 2: a = 1, b = 1 -- one pixel outward, the box's own edge; width 3: a = 1, b = 2 -- one outward, the edge, one inward
    for width, a, b in [(2, 1, 1), (3, 1, 2), (6, 3, 3), (7, 3, 4)]:
        outer = (xs >= 10 - a) & (xs <= 30 + a) & (ys >= 12 - a) & (ys <= 25 + a)
        inner = (xs >= 10 + b) & (xs <= 30 - b) & (ys >= 12 + b) & (ys <= 25 - b)
        got = ref.ring_alpha(48, 64, box, width) == 256
        assert np.array_equal(got, outer & ~inner)
        assert got.sum() == (21 + 2 * a) * (14 + 2 * a) - max(21 - 2 * b, 0) * max(14 - 2 * b, 0)
    assert ref.ring_alpha(48, 64, (30, 12, 10, 25), 3).sum() == 0              # x1 < x0 draws nothing
    assert ref.ring_alpha(48, 64, (10, 25, 30, 12), 1).sum() == 0


@pytest.mark.parametrize("var,t", [(4.0, 2), (25.0, 3), (100.0, 3), (100.0, 1)])     # ratios 0.9998, 1.0019, 0.9948, 1.0017
def test_isotropic_ellipse_has_the_contours_area(var, t):
    n = 257
    a = ref.ellipse_alpha(n, n, n // 2, n // 2, [[var, 0.0], [0.0, var]], t, R2)
    want = 2 * math.pi * math.sqrt(R2 * var) * t
    assert abs(_alpha_sum(a) / want - 1) < 0.02, (_alpha_sum(a), want)
    assert a.min() >= 0 and a.max() <= 256 and a[n // 2, n // 2] == 0


def test_ellipse_half_turn_symmetry_extent_and_skips():
    n = 161
    for cov, t in [([[30.0, 12.0], [12.0, 9.0]], 2), ([[400.0, 0.0], [0.0, 1.0]], 3), ([[2.0, -1.5], [-1.5, 7.0]], 1)]:
        a = ref.ellipse_alpha(n, n, n // 2, n // 2, cov, t, R2)
        assert a.sum() > 0 and np.array_equal(a, a[::-1, ::-1])
    # S = diag(400, 1): the first-order distance reaches beyond r*sqrt(a) = 49.7 along x, inside the extent's factor 1.5
    a = ref.ellipse_alpha(n, n, n // 2, n // 2, [[400.0, 0.0], [0.0, 1.0]], 1, R2)
    reach = np.abs(np.nonzero(a.any(axis=0))[0] - n // 2).max()
    assert 50 <= reach <= math.ceil(1.5 * math.sqrt(R2 * 400.0)) + 1 + 1
    for bad in ([[1.0, 2.0], [2.0, 1.0]], [[-1.0, 0.0], [0.0, 1.0]], [[1.0, 0.0], [0.0, 0.0]], [[np.nan, 0.0], [0.0, 1.0]],
                [[1.0, np.inf], [np.inf, 1.0]], [[4.0, 2.0], [2.0, 1.0]]):
        assert ref.ellipse_alpha(n, n, 5, 5, bad, 2, R2) is None
    # clipped: a centre outside the frame still covers what reaches in, one far away covers nothing
    assert ref.ellipse_alpha(20, 20, -3, -3, [[25.0, 0.0], [0.0, 25.0]], 2, R2).sum() > 0
    assert ref.ellipse_alpha(20, 20, -300, 5, [[25.0, 0.0], [0.0, 25.0]], 2, R2).sum() == 0


def test_colour_ramp():
    r = ref.ramp().astype(int)
    assert r.shape == (256, 3)
    assert tuple(r[0]) == (0, 0, 128) and tuple(r[255]) == (127, 0, 0)
    assert tuple(r[128]) == (130, 255, 125)
    d = np.diff(r, axis=0)
    # blue rises then holds then falls; green and red rise, hold, fall: each channel is unimodal
    for c in range(3):
        s = np.sign(d[:, c])
        s = s[s != 0]
        assert np.all(np.diff(s) <= 0), c
    assert len({tuple(v) for v in r}) == 256                                   # every index has its own colour
    black = ref.heat_colour(np.zeros((1, 256, 3), np.uint8), np.arange(256)[None, :])
    assert len({tuple(v) for v in black[0]}) == 256                            # ... and still after the 0.9 blend onto black


def test_painters_order_and_blend():
    frame = np.full((40, 40, 3), 77, np.uint8)
    boxes = [(5, 5, 20, 20), (5, 5, 20, 20)]
    covs = np.tile(np.array([[9.0, 0.0], [0.0, 9.0]], np.float32), (2, 2, 1, 1))
    colors = [(255, 0, 0), (0, 0, 255)]
    out, skipped = ref.overlay(frame, boxes, covs, colors, line_width=2, labels=False)
    assert skipped == 0 and tuple(out[5, 10]) == (0, 0, 255)                   # the later detection's ring is on top
    rev, _ = ref.overlay(frame, boxes, covs, colors[::-1], line_width=2, labels=False)
    assert tuple(rev[5, 10]) == (255, 0, 0)
    gt, _ = ref.overlay(frame, [], np.zeros((0, 2, 2, 2)), np.zeros((0, 3)), gt_boxes=[(1, 1, 8, 8)])
    assert tuple(gt[1, 4]) == (0, 255, 0) and tuple(gt[4, 4]) == (77, 77, 77)
    img = np.array([[[10, 200, 255]]], np.uint8)
    ref.blend(img, np.array([[128]]), (255, 0, 0))
    assert tuple(img[0, 0]) == ((10 * 128 + 255 * 128 + 128) >> 8, (200 * 128 + 128) >> 8, (255 * 128 + 128) >> 8)


@pytest.fixture(scope="module")
def lib():
    from bayes_od_rc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("the library is not built")
    return _lib.load()


def test_font_through_the_library(lib):
    from bayes_od_rc_amd import render
    f = render.font()
    assert f.shape == (41, 7, 5) and len(render.CHARSET) == 41 and set(np.unique(f)) <= {0, 1}
    space = render.CHARSET.index(' ')
    keys = set()
    for k in range(41):
        assert (f[k].sum() == 0) == (k == space), render.CHARSET[k]
        keys.add(f[k].tobytes())
    assert len(keys) == 41
    assert list(render.encode_text("Car 0.97")[:9]) == [2, 0, 17, 37, 26, 36, 35, 33, 0xFF]
    assert list(render.encode_text("A#b")[:4]) == [0, 40, 1, 0xFF]
    assert (render.encode_text("x" * 40) == 23).all()
    st = lib.bod_render_font(None, None)
    assert st == 1 and b"bod_render_font" in lib.bod_last_error(None)


def test_detections_from_tree(tmp_path):
    from bayes_od_rc_amd import render
    for d in ('mean', 'cov', 'cov_epistemic', 'cat_param'):
        os.makedirs(tmp_path / d)
    mean = np.array([[30.0, 40.0, 10.0, 20.0], [8.5, 9.5, 4.0, 6.0], [20.0, 20.0, 2.0, 2.0]])
    s = np.array([[4.0, 1.0, 0.5, 0.0], [1.0, 9.0, 0.0, 2.0], [0.5, 0.0, 16.0, 3.0], [0.0, 2.0, 3.0, 36.0]])
    cov = np.stack([s, 2 * s, s])
    cat = np.array([[0.1, 0.85, 0.05], [0.6, 0.3, 0.1], [0.3, 0.3, 0.4]])
    np.save(tmp_path / 'mean' / 'f0.npy', mean)
    np.save(tmp_path / 'cov' / 'f0.npy', cov)
    np.save(tmp_path / 'cov_epistemic' / 'f0.npy', 0.25 * cov)
    np.save(tmp_path / 'cat_param' / 'f0.npy', cat)
    det = render.detections_from_tree(str(tmp_path), 'f0', min_score=0.5, cov_scale=3.0, categories=['car', 'Person'])
    assert det.boxes.tolist() == [[30, 25, 50, 35], [6, 6, 12, 10]]            # x0 y0 x1 y1, truncated
    # by hand, (v, u, h, w) -> corner: v1 = v - h/2, u1 = u - w/2 ; v2 = v + h/2, u2 = u + w/2
    #   var(u1) = S_uu + S_ww/4 - S_uw = 9 + 9 - 2 = 16      var(v1) = S_vv + S_hh/4 - S_vh = 4 + 4 - 0.5 = 7.5
    #   cov(u1, v1) = S_uv - S_uh/2 - S_wv/2 + S_wh/4 = 1 - 0 - 0 + 0.75 = 1.75
    #   var(u2) = 9 + 9 + 2 = 20    var(v2) = 4 + 4 + 0.5 = 8.5    cov(u2, v2) = 1 + 0 + 0 + 0.75 = 1.75
    tl = 3.0 * np.array([[16.0, 1.75], [1.75, 7.5]])
    br = 3.0 * np.array([[20.0, 1.75], [1.75, 8.5]])
    np.testing.assert_allclose(det.corner_covs[0], [tl, br], rtol=1e-6)
    np.testing.assert_allclose(det.corner_covs[1], [2 * tl, 2 * br], rtol=1e-6)
    assert det.corner_covs.dtype == np.float32 and det.boxes.dtype == np.int32
    assert det.colors.tolist() == [list(render.PALETTE[1]), list(render.PALETTE[0])]
    assert bytes(det.text[0][:12]) == bytes(render.encode_text("person 0.85")[:12]) and det.text[0][11] == 0xFF
    assert bytes(det.text[1][:8]) == bytes(render.encode_text("car 0.60")[:8])
    part = render.detections_from_tree(str(tmp_path), 'f0', min_score=0.5, cov_scale=3.0, cov_dir='cov_epistemic')
    np.testing.assert_allclose(part.corner_covs, 0.25 * det.corner_covs, rtol=1e-6)
    assert bytes(part.text[0][:6]) == bytes(render.encode_text("1 0.85")[:6])
    none = render.detections_from_tree(str(tmp_path), 'f0', min_score=0.99)
    assert none.boxes.shape == (0, 4) and none.corner_covs.shape == (0, 2, 2, 2) and none.text.shape == (0, 16)


def _call(lib, n=1, hw=((4, 5),), num_det=(1,), boxes=((0, 0, 2, 2),), covs=None, colors=((1, 2, 3),), text=None, num_gt=None, gt=None,
          view=0, line_width=2, labels=1, r2=R2, null=()):
    from bayes_od_rc_amd import _lib
    u8 = C.POINTER(C.c_uint8)
    d = int(sum(num_det))
    arr = {
        'in': np.zeros(max(1, sum(3 * h * w for h, w in hw)), np.uint8), 'hw': np.asarray(hw, np.int32).reshape(-1, 2),
        'num_det': np.asarray(num_det, np.int32), 'boxes': np.asarray(boxes, np.int32).reshape(-1, 4),
        'covs': np.asarray(covs if covs is not None else np.tile(np.eye(2, dtype=np.float32), (max(d, 1), 2, 1, 1)), np.float32),
        'colors': np.asarray(colors, np.uint8).reshape(-1, 3), 'text': None if text is None else np.asarray(text, np.uint8).reshape(-1, 16),
        'num_gt': None if num_gt is None else np.asarray(num_gt, np.int32), 'gt': None if gt is None else np.asarray(gt, np.int32).reshape(-1, 4),
    }
    arr['out'] = np.zeros_like(arr['in'])
    for k in null:
        arr[k] = None
    p = lambda k, t: None if arr[k] is None else arr[k].ctypes.data_as(t)      # noqa: E731
    opt = _lib.BodRenderOptions(view, line_width, labels, r2, (C.c_int32 * 4)(0, 0, 0, 0))
    st = lib.bod_render_frames_u8(0, n, p('in', u8), p('hw', _lib._I), p('num_det', _lib._I), p('boxes', _lib._I), p('covs', _lib._F),
                                  p('colors', u8), p('text', u8), p('num_gt', _lib._I), p('gt', _lib._I), C.byref(opt), p('out', u8), None)
    return st, lib.bod_last_error(None)


def test_argument_validation_needs_no_device(lib):
    from bayes_od_rc_amd import _lib
    bad = _lib.BOD_ERR_INVALID_ARG
    st, msg = _call(lib, n=-1)
    assert st == bad and b"n = -1" in msg
    st, msg = _call(lib, n=0, null=('in', 'hw', 'num_det', 'boxes', 'covs', 'colors', 'out'))
    assert st == _lib.BOD_OK and msg == b""
    for name in ('in', 'hw', 'num_det', 'out', 'boxes', 'covs', 'colors'):
        st, msg = _call(lib, null=(name,))
        assert st == bad and b"NULL" in msg, name
    st, msg = _call(lib, num_gt=(2,), gt=None)
    assert st == bad and b"gt_boxes is NULL" in msg
    for t in (0, 8, -3):
        st, msg = _call(lib, line_width=t)
        assert st == bad and b"line_width" in msg
    for r2 in (0.0, -1.0, float('nan'), float('inf')):
        st, msg = _call(lib, r2=r2)
        assert st == bad and b"r2" in msg
    st, msg = _call(lib, view=2)
    assert st == bad and b"unknown view 2" in msg
    text = np.full((3, 16), 0xFF, np.uint8)
    text[0, :3] = (0, 40, 5)
    text[2, :2] = (7, 41)
    st, msg = _call(lib, n=2, hw=((4, 5), (3, 3)), num_det=(1, 2), boxes=[(0, 0, 2, 2)] * 3, colors=[(1, 2, 3)] * 3, text=text)
    assert st == bad and b"frame 1 row 1" in msg and b"glyph index 41" in msg
    st, msg = _call(lib, hw=((0, 5),))
    assert st == bad and b"frame 0 is 0x5" in msg
    st, msg = _call(lib, num_det=(-1,))
    assert st == bad and b"frame 0" in msg
    # valid arguments get past the validation: without a device the call then fails loudly, it never falls back
    import torch
    if not torch.cuda.is_available():
        st, msg = _call(lib)
        assert st == _lib.BOD_ERR_NO_DEVICE and b"no CPU fallback" in msg
