"""GPU: the rendering stage (csrc/render_kernels.hip) through bod_render_frames_u8 against tests/render_reference.py.
OVERLAY is byte-equal.  HEAT's index plane and output are equal outside the pixels the CPU heatmaps cannot decide (below).

Sizes: the paint kernel works on 32 x 32 tiles with 4 pixels per thread, 64 primitive records per LDS chunk.  Every call renders a
48 x 64 frame (2 x 2 tiles, the lower row ragged) and a 37 x 53 one (ragged both ways, rows that are not 4-byte aligned) in one
batch; the stacked case puts 70 labelled detections -- over 1400 primitives -- on one tile."""
import numpy as np
import pytest

import conftest  # noqa: F401
import render_reference as ref

pytestmark = pytest.mark.gpu

R2 = 6.180074
SIZES = [(48, 64), (37, 53)]
FLOOR = 0.0027


def frames():
    rng = np.random.RandomState(11)
    return [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in SIZES]


def _render():
    from bayes_od_rc_amd import render
    return render


def _cov(sx, sy, rho=0.0):
    return [[sx * sx, rho * sx * sy], [rho * sx * sy, sy * sy]]


def _dets(rows):
    """rows: (box, cov_tl, cov_br, colour, label)."""
    r = _render()
    return r.make_detections([x[0] for x in rows], [[x[1], x[2]] for x in rows], [x[3] for x in rows], [x[4] for x in rows])


def _random_rows(seed, count, h, w, lo=(0, 0), hi=None):
    rng = np.random.RandomState(seed)
    hi = hi or (w, h)
    rows = []
    for i in range(count):
        x0, y0 = rng.randint(lo[0], hi[0] - 6), rng.randint(lo[1], hi[1] - 6)
        x1, y1 = rng.randint(x0 + 2, hi[0]), rng.randint(y0 + 2, hi[1])
        rows.append(((x0, y0, x1, y1), _cov(rng.uniform(0.5, 4), rng.uniform(0.5, 4), rng.uniform(-0.8, 0.8)),
                     _cov(rng.uniform(0.5, 4), rng.uniform(0.5, 4), rng.uniform(-0.8, 0.8)), tuple(rng.randint(0, 256, 3)),
                     "%s %.2f" % (("car", "person", "traffic_light-x")[i % 3], rng.uniform(0, 1))))
    return rows


def _cases():
    """name -> (rows of frame 0, rows of frame 1, gt boxes per frame or None, options)."""
    red, blue, white = (255, 30, 30), (40, 90, 255), (250, 250, 250)
    c = {}
    c["none"] = ([], [], None, {})
    c["one"] = ([((10, 8, 40, 30), _cov(3, 2, 0.5), _cov(2, 4, -0.3), red, "car 0.91")], [], None, {})
    c["five_overlapping"] = (_random_rows(1, 5, 48, 64), _random_rows(2, 5, 37, 53), [[(3, 3, 30, 30), (20, 10, 60, 44)], []], {})
    c["stacked_70_on_one_tile"] = (_random_rows(3, 70, 48, 64, hi=(32, 32)), _random_rows(4, 3, 37, 53), None, {})
    c["tile_corner"] = ([((32, 32, 63, 47), _cov(5, 3, 0.6), _cov(2, 2), blue, "")],
                        [((0, 0, 32, 32), _cov(1, 1), _cov(6, 2, -0.7), red, "x")], None, {"line_width": 3})
    c["every_edge_and_outside"] = (
        [((-5, -4, 67, 50), _cov(6, 5, 0.4), _cov(5, 7, -0.5), white, "person 0.50"),
         ((-500, -500, -400, -400), _cov(3, 3), _cov(3, 3), red, "car 1.00"),
         ((1000, 1000, 1100, 1100), _cov(3, 3), _cov(3, 3), red, "car 1.00"),
         ((-2 ** 31, -2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1), _cov(3, 3), _cov(3, 3), blue, "far 0.10")],
        [((-3, 10, 55, 20), _cov(8, 1), _cov(1, 8), blue, "truck 0.77"), ((20, -6, 30, 40), _cov(2, 2), _cov(2, 2), red, "")],
        [[(-10, -10, 70, 60)], [(50, 30, 60, 40)]], {"line_width": 4})
    for t in (1, 3, 7):
        c["line_width_%d" % t] = (_random_rows(5, 4, 48, 64), _random_rows(6, 4, 37, 53), [[(5, 5, 25, 25)], [(1, 1, 51, 35)]], {"line_width": t})
    c["wide_ellipse_reaches_its_extent"] = ([((64, 24, 70, 30), [[400.0, 0.0], [0.0, 1.0]], _cov(1, 1), white, "")],
                                            [((26, 18, 40, 30), [[400.0, 0.0], [0.0, 1.0]], [[1.0, 0.0], [0.0, 400.0]], red, "")], None,
                                            {"line_width": 1})
    nan = float("nan")
    c["skipped_ellipses"] = (
        [((5, 5, 30, 30), [[1.0, 2.0], [2.0, 1.0]], _cov(2, 2), red, "car 0.10"),              # det < 0
         ((8, 20, 50, 40), [[-1.0, 0.0], [0.0, 1.0]], [[4.0, 2.0], [2.0, 1.0]], blue, "bus 0.20"),  # negative variance; det == 0
         ((12, 2, 60, 12), [[nan, 0.0], [0.0, 1.0]], [[1.0, nan], [nan, 1.0]], white, "nan 0.30")],
        [((4, 4, 20, 20), _cov(2, 2), [[1.0, 0.0], [0.0, float("inf")]], red, "inf")], None, {})
    c["labels"] = ([((2, 2, 20, 12), _cov(1, 1), _cov(1, 1), red, ""), ((2, 14, 20, 24), _cov(1, 1), _cov(1, 1), blue, "a"),
                    ((1, 26, 60, 36), _cov(1, 1), _cov(1, 1), white, "0123456789abcdef"),
                    ((30, 38, 62, 46), _cov(1, 1), _cov(1, 1), red, "clipped_right.%-_")],
                   [((40, 30, 52, 36), _cov(1, 1), _cov(1, 1), blue, "bottom right 9")], None, {})
    c["labels_off"] = (c["labels"][0], c["labels"][1], None, {"labels": False})
    c["r2_other"] = (_random_rows(7, 3, 48, 64), [], None, {"r2": 2.2957, "line_width": 2})
    return c


CASES = _cases()
EXPECTED_SKIPS = {"skipped_ellipses": [5, 1]}


def _want(frame, det, gt, opts):
    return ref.overlay(frame, det.boxes, det.corner_covs, det.colors, det.text, gt, opts.get("line_width", 2), opts.get("labels", True),
                       opts.get("r2", R2), _render().font())


@pytest.mark.parametrize("name", sorted(CASES))
def test_overlay_is_byte_equal(name):
    rows0, rows1, gt, opts = CASES[name]
    fr = frames()
    dets = [_dets(rows0), _dets(rows1)]
    got, skipped = _render().render_frames(fr, dets, view="overlay", gt_boxes=gt, return_skipped=True, **opts)
    for i in range(2):
        want, want_skipped = _want(fr[i], dets[i], gt[i] if gt is not None else None, opts)
        bad = np.argwhere((got[i] != want).any(axis=2))
        assert len(bad) == 0, (name, i, len(bad), bad[:5], got[i][tuple(bad[0])], want[tuple(bad[0])])
        assert skipped[i] == want_skipped
        if name in EXPECTED_SKIPS:
            assert skipped[i] == EXPECTED_SKIPS[name][i]
    if name == "none":
        assert all(np.array_equal(a, b) for a, b in zip(got, fr))
    else:
        assert (got[0] != fr[0]).any()


def test_a_frame_does_not_depend_on_its_batch():
    rows0, rows1, gt, opts = CASES["five_overlapping"]
    fr = frames()
    r = _render()
    both = r.render_frames(fr, [_dets(rows0), _dets(rows1)], gt_boxes=gt)
    alone = r.render_frames([fr[1]], [_dets(rows1)], gt_boxes=[gt[1]])
    swapped = r.render_frames([fr[1], fr[0]], [_dets(rows1), _dets(rows0)], gt_boxes=[gt[1], gt[0]])
    assert np.array_equal(both[1], alone[0]) and np.array_equal(both[1], swapped[0]) and np.array_equal(both[0], swapped[1])
    assert r.render_frames([], []) == []


# HEAT: two overlapping detections and one touching the frame's border
# (small boxes against their sigmas: a heatmap that saturates at 1.0 puts whole plateaus on the integer 255.0, which no comparison of
# truncations can decide)
HEAT_BOXES = [(30, 28, 38, 36), (35, 33, 44, 41), (54, 6, 63, 15)]
HEAT_COVS = [[_cov(1.5, 1.4, 0.3), _cov(1.6, 1.5, -0.2)], [_cov(1.7, 1.5), _cov(1.6, 1.8, 0.5)], [_cov(1.4, 1.6, -0.4), _cov(1.5, 1.7)]]
HEAT_EXEMPT_CPU = 1


def _heat_exempt(hm_cpu, hm_gpu=None):
    """Pixels the comparison cannot decide: a CPU heatmap value whose h*255 lies within 1e-3 of an integer (a last-bit difference of
    the CDF moves the truncation), or, with the device's maps, a pixel on the 0.0027 floor's boundary as test_gpu_pdq's _maps_close
    excuses it."""
    v = hm_cpu.astype(np.float64) * 255.0
    ex = ((np.abs(v - np.rint(v)) <= 1e-3) & (hm_cpu != 0)).any(axis=0)
    if hm_gpu is not None:
        bad = np.abs(hm_gpu.astype(np.float64) - hm_cpu) > 1e-6
        floor = bad & ((hm_gpu == 0) | (hm_cpu == 0)) & ((np.abs(hm_gpu - FLOOR) <= 1e-6) | (np.abs(hm_cpu - FLOOR) <= 1e-6))
        assert not (bad & ~floor).any()
        ex |= floor.any(axis=0)
    return ex


def test_heat_view():
    """The CPU restatement alone leaves 1 pixel (HEAT_EXEMPT_CPU) of the 3072 undecided at these thresholds: counted by this test on
    the CPU heatmaps before anything is compared.  The cap for the comparison is 0.5 % = 15 pixels, a quarter of it 3."""
    from bayes_od_rc_amd import engine
    r = _render()
    h, w = SIZES[0]
    fr = frames()
    det = r.make_detections(HEAT_BOXES, HEAT_COVS)
    hm = ref.box_heatmaps((h, w), det.boxes, det.corner_covs)
    cpu_only = int(_heat_exempt(hm).sum())
    print("HEAT: pixels the CPU heatmaps leave undecided:", cpu_only)
    assert cpu_only <= HEAT_EXEMPT_CPU <= (h * w * 5 // 1000) // 4
    assert (hm[0] != 0).any() and ((hm[0] != 0) & (hm[1] != 0)).any() and (hm[2][:, w - 1] != 0).any()
    empty = r.make_detections()
    got = r.render_frames([fr[0], fr[1], np.zeros((h, w, 3), np.uint8)], [det, empty, det], view="heat")
    # the index plane, read back from the render onto black: every index has its own colour there (test_render_host.py)
    black = ref.heat_colour(np.zeros((1, 256, 3), np.uint8), np.arange(256)[None, :])[0]
    lut = {tuple(v): i for i, v in enumerate(black)}
    index = np.array([[lut[tuple(p)] for p in row] for row in got[2]])
    want_index = ref.heat_index(hm, (h, w))
    _, _, _, gpu_hm = engine.pdq_frames((h, w), [0], np.zeros((0, 4), np.int32), [3], det.boxes, det.corner_covs.astype(np.float64), device=0,
                                        heatmaps=True)
    exempt = _heat_exempt(hm, np.asarray(gpu_hm).reshape(3, h, w))
    print("HEAT: exempt pixels with the device's maps:", int(exempt.sum()))
    assert exempt.sum() <= h * w * 5 // 1000
    assert np.array_equal(index[~exempt], want_index[~exempt])
    assert np.array_equal(got[0][~exempt], ref.heat_colour(fr[0], want_index)[~exempt])
    # ... and exactly the device's own maps everywhere
    dev_index = ref.heat_index(np.asarray(gpu_hm).reshape(3, h, w), (h, w))
    assert np.array_equal(index, dev_index) and np.array_equal(got[0], ref.heat_colour(fr[0], dev_index))
    # a frame without detections is the ramp's index 0 blended in
    assert np.array_equal(got[1], ref.heat_colour(fr[1], np.zeros(SIZES[1], np.int64)))


def _status(**kw):
    import test_render_host as host
    from bayes_od_rc_amd import _lib
    return host._call(_lib.load(), **kw)


def test_errors_name_frame_and_row():
    from bayes_od_rc_amd import _lib
    bad = _lib.BOD_ERR_INVALID_ARG
    assert _status(n=-1)[0] == bad
    assert _status(n=0, null=("in", "hw", "num_det", "boxes", "covs", "colors", "out"))[0] == _lib.BOD_OK
    for name in ("in", "hw", "num_det", "out", "boxes", "covs", "colors"):
        st, msg = _status(null=(name,))
        assert st == bad and b"NULL" in msg
    assert _status(num_gt=(1,), gt=None)[0] == bad
    for kw, word in [({"line_width": 0}, b"line_width"), ({"line_width": 8}, b"line_width"), ({"r2": 0.0}, b"r2"),
                     ({"r2": float("nan")}, b"r2"), ({"r2": float("inf")}, b"r2"), ({"view": 7}, b"unknown view 7")]:
        st, msg = _status(**kw)
        assert st == bad and word in msg, kw
    text = np.full((3, 16), 0xFF, np.uint8)
    text[2, :2] = (7, 200)
    st, msg = _status(n=2, hw=((4, 5), (3, 3)), num_det=(1, 2), boxes=[(0, 0, 2, 2)] * 3, colors=[(1, 2, 3)] * 3, text=text)
    assert st == bad and b"frame 1 row 1" in msg and b"glyph index 200" in msg
    # HEAT refuses the rows bod_pdq_frames refuses, by frame and row, and draws nothing
    r = _render()
    fr = frames()
    good = (10, 8, 30, 26)
    for covs, word in [([_cov(2, 2), [[1.0, 0.0], [0.0, -1.0]]], "non-positive variance"),
                       ([[[float("nan"), 0.0], [0.0, 1.0]], _cov(2, 2)], "non-finite"),
                       ([[[1.0, 3.0], [3.0, 1.0]], _cov(2, 2)], "correlation")]:
        det = r.make_detections([good, good], [[_cov(2, 2), _cov(2, 2)], covs])
        with pytest.raises(ValueError, match="frame 1 row 1: .*" + word):
            r.render_frames(fr, [r.make_detections(), det], view="heat")
    with pytest.raises(ValueError, match="frame 0 row 0: .*outside"):
        r.render_frames(fr[:1], [r.make_detections([(500, 500, 600, 600)], [[_cov(2, 2), _cov(2, 2)]])], view="heat")
    # a valid call right after: the library is as it was
    out = r.render_frames(fr[:1], [r.make_detections([good], [[_cov(2, 2), _cov(2, 2)]])], view="heat")
    assert out[0].shape == fr[0].shape
