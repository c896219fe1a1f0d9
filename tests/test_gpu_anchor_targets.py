"""GPU: anchor-target assignment on the device (target_kernels.hip, bod_anchor_targets) against the host generator
(sample_builder.create_sample_dict, which tests/test_geometry.py pins to the oracle's).  Masks, best GT, best IoU, class
targets and the two linear box-target columns are IEEE add / multiply / divide / compare in a fixed order, so they are compared
for equality, every anchor included; the two logarithmic columns are held to 4 fp32 ulps of float64."""
import ctypes

import numpy as np
import pytest

from conftest import ANCHOR_CFG

pytestmark = pytest.mark.gpu

SIZES = [(512, 512), (720, 1280), (384, 1248), (100, 310)]       # the last has ragged top levels (ceil'd anchor counts)


def _random_frame(hw, g, seed, num_classes=8):
    """The recipe of the issue: one generator per frame, G values at a time in the order y1, x1, h, w."""
    rng = np.random.default_rng(seed)
    h_im, w_im = hw
    y1 = rng.uniform(0, 0.7 * h_im, g)
    x1 = rng.uniform(0, 0.7 * w_im, g)
    h = rng.uniform(12, 0.3 * h_im, g)
    w = rng.uniform(12, 0.3 * w_im, g)
    boxes = np.stack([y1, x1, y1 + h, x1 + w], axis=1).astype(np.float32)
    classes = np.eye(num_classes, dtype=np.float32)[rng.integers(0, num_classes - 1, g)]
    return boxes, classes


def _host(hw, boxes, classes, cfg=ANCHOR_CFG):
    """Host targets of one frame: the sample dict's own arrays, plus the best GT / best IoU from the same functions."""
    from bayes_od_rc_amd import box_utils
    from bayes_od_rc_amd.anchor_generator import FpnAnchorGenerator
    from bayes_od_rc_amd.sample_builder import create_sample_dict
    sample = create_sample_dict(np.zeros(hw + (3,), np.float32), cfg, boxes, classes)
    anchors = sample["anchors"]
    ious = box_utils.bbox_iou_vuvu(box_utils.vuhw_to_vuvu_np(anchors), boxes)
    assert ious.dtype == np.float32
    pos, neg, arg = FpnAnchorGenerator.positive_negative_batching(ious, cfg["min_positive_iou"], cfg["max_negative_iou"])
    assert np.array_equal(pos, sample["positive_anchors_mask"]) and np.array_equal(neg, sample["negative_anchors_mask"])
    return {"anchors": anchors, "pos": pos, "neg": neg, "best_gt": arg.astype(np.int32), "best_iou": ious[np.arange(len(arg)), arg],
            "cls": sample["anchors_class_targets"], "box": sample["anchors_box_targets"], "ious": ious}


def _ulps_from_float64_log(box_t, anchors, boxes, best_gt):
    """Columns 2, 3 against float64 5*log(q), q the fp32 quotient (itself exact): error in fp32 ulps of that value."""
    gt = boxes[best_gt]
    worst = 0.0
    for col, (lo, hi, dim) in enumerate([(0, 2, 2), (1, 3, 3)]):
        q = ((gt[:, hi] - gt[:, lo]) / anchors[:, dim]).astype(np.float32)
        assert q.dtype == np.float32
        ref = 5.0 * np.log(q.astype(np.float64))
        ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
        err = np.abs(box_t[:, 2 + col].astype(np.float64) - ref) / ulp
        worst = max(worst, float(err.max()))
    return worst


def _compare(hw, frames, got, refs=None):
    cls_t, box_t, pos, neg, best_gt, best_iou = got
    worst = 0.0
    for b, (boxes, classes) in enumerate(frames):
        ref = refs[b] if refs is not None else _host(hw, boxes, classes)
        assert np.array_equal(pos[b], ref["pos"]), (hw, b)
        assert np.array_equal(neg[b], ref["neg"]), (hw, b)
        assert np.array_equal(best_gt[b], ref["best_gt"]), (hw, b)
        assert np.array_equal(cls_t[b], ref["cls"]), (hw, b)
        assert np.array_equal(best_iou[b], ref["best_iou"]), (hw, b)
        assert np.array_equal(box_t[b][:, :2], ref["box"][:, :2]), (hw, b)
        ulps = _ulps_from_float64_log(box_t[b], ref["anchors"], boxes, ref["best_gt"])
        worst = max(worst, ulps)
    return worst


@pytest.mark.parametrize("hw", SIZES)
def test_random_frames_match_the_host_generator(hw):
    """B = 3 frames with G = 5, 12, 30 in one call and G = 200 in another; equality on everything but the log columns,
    which stay within 4 fp32 ulps of float64 (logf is a 1-ulp function and the *5 rounds once more)."""
    from bayes_od_rc_amd.anchor_generator import FpnAnchorGenerator
    from bayes_od_rc_amd.engine import anchor_targets
    anchors = FpnAnchorGenerator(ANCHOR_CFG).generate_all(hw + (3,)).astype(np.float32)
    calls = [[_random_frame(hw, g, seed) for g, seed in ((5, 7), (12, 8), (30, 9))],
             [_random_frame(hw, 200, 10), _random_frame(hw, 200, 11)]]
    worst = 0.0
    for frames in calls:
        # so that the comparison cannot pass on nothing (minima of the host generator alone on these cases: 29 and 73)
        refs = []
        for boxes, classes in frames:
            ref = _host(hw, boxes, classes)
            del ref["ious"]
            refs.append(ref)
            assert ref["pos"].sum() >= 20 and (~ref["pos"] & ~ref["neg"]).sum() >= 50, (hw, len(boxes), ref["pos"].sum())
        got = anchor_targets(anchors, [f[0] for f in frames], [f[1] for f in frames], ANCHOR_CFG["min_positive_iou"],
                             ANCHOR_CFG["max_negative_iou"], return_best=True)
        assert got[0].shape == (len(frames), anchors.shape[0], 8) and got[1].shape == (len(frames), anchors.shape[0], 4)
        worst = max(worst, _compare(hw, frames, got, refs))
    print("%dx%d: worst log-column error %.2f fp32 ulps of float64" % (hw[0], hw[1], worst))
    assert worst <= 4.0, worst


def test_constructed_rows():
    """A GT equal to an anchor's own corners (the area quirk makes that IoU about 1.3), one box twice with two classes (the
    first row wins the tie), a box wholly outside the image -- and a frame whose only GT is the handlers' placeholder."""
    from bayes_od_rc_amd import box_utils
    from bayes_od_rc_amd.anchor_generator import FpnAnchorGenerator
    from bayes_od_rc_amd.engine import anchor_targets
    hw = (128, 128)
    anchors = FpnAnchorGenerator(ANCHOR_CFG).generate_all(hw + (3,)).astype(np.float32)
    k = int(np.nonzero((anchors[:, 0] == 60.0) & (anchors[:, 1] == 68.0))[0][0])          # a level-3 anchor inside the image
    own = box_utils.vuhw_to_vuvu_np(anchors[k:k + 1])[0]
    twice = np.asarray([20.0, 30.0, 70.0, 90.0], np.float32)
    outside = np.asarray([600.0, 600.0, 700.0, 700.0], np.float32)
    boxes = np.stack([twice, own, twice, outside]).astype(np.float32)
    classes = np.eye(8, dtype=np.float32)[[2, 0, 5, 3]]
    placeholder = (np.asarray([[0.0, 0.0, 1.0, 1.0]], np.float32), np.eye(8, dtype=np.float32)[[7]])
    frames = [(boxes, classes), placeholder]
    ref = _host(hw, boxes, classes)
    assert 1.2 < ref["ious"][k, 1] < 1.4 and ref["best_gt"][k] == 1 and ref["pos"][k]
    assert np.array_equal(ref["ious"][:, 0], ref["ious"][:, 2]) and not np.any(ref["best_gt"] == 2)      # the tie goes to the first row
    assert (ref["pos"] & (ref["best_gt"] == 0)).sum() > 0 and np.all(ref["cls"][ref["pos"] & (ref["best_gt"] == 0)] == classes[0])
    assert np.all(ref["ious"][:, 3] == 0) and not np.any(ref["best_gt"] == 3)
    ref_p = _host(hw, *placeholder)
    assert not ref_p["pos"].any() and ref_p["neg"].all() and not ref_p["best_gt"].any()
    got = anchor_targets(anchors, [f[0] for f in frames], [f[1] for f in frames], return_best=True)
    worst = _compare(hw, frames, got)
    assert worst <= 4.0, worst
    assert not got[2][1].any() and got[3][1].all() and not got[4][1].any()
    assert np.all(got[0][1] == np.eye(8, dtype=np.float32)[7])


def test_other_class_counts_and_thresholds():
    """C = 4 (KITTI's rows) takes the 16-byte class-row path, C = 3 the scalar one; thresholds are the call's, not constants."""
    from bayes_od_rc_amd.anchor_generator import FpnAnchorGenerator
    from bayes_od_rc_amd.engine import anchor_targets
    hw = (100, 310)
    anchors = FpnAnchorGenerator(ANCHOR_CFG).generate_all(hw + (3,)).astype(np.float32)
    for c in (4, 3):
        cfg = dict(ANCHOR_CFG, min_positive_iou=0.6, max_negative_iou=0.3)
        frames = [_random_frame(hw, 12, 21, num_classes=c), _random_frame(hw, 5, 22, num_classes=c)]
        got = anchor_targets(anchors, [f[0] for f in frames], [f[1] for f in frames], 0.6, 0.3, return_best=True)
        for b, (boxes, classes) in enumerate(frames):
            ref = _host(hw, boxes, classes, cfg)
            assert ref["pos"].sum() > 0
            assert np.array_equal(got[2][b], ref["pos"]) and np.array_equal(got[3][b], ref["neg"])
            assert np.array_equal(got[0][b], ref["cls"]) and np.array_equal(got[4][b], ref["best_gt"])


def test_bad_arguments_are_refused_before_anything_runs():
    from bayes_od_rc_amd import _lib
    from bayes_od_rc_amd.anchor_generator import FpnAnchorGenerator
    from bayes_od_rc_amd.engine import anchor_targets
    lib = _lib.load()
    hw = (100, 310)
    anchors = FpnAnchorGenerator(ANCHOR_CFG).generate_all(hw + (3,)).astype(np.float32)
    a = anchors.shape[0]
    boxes, classes = _random_frame(hw, 5, 7)
    with pytest.raises(ValueError, match="ground-truth rows"):
        anchor_targets(anchors, [boxes, np.zeros((0, 4), np.float32)], [classes, np.zeros((0, 8), np.float32)])
    with pytest.raises(ValueError, match="C = 1"):
        anchor_targets(anchors, [boxes], [np.ones((5, 1), np.float32)])
    u8 = ctypes.POINTER(ctypes.c_uint8)
    ng = np.asarray([5], np.int32)
    outs = {"cls": np.full((1, a, 8), -7.0, np.float32), "box": np.full((1, a, 4), -7.0, np.float32),
            "pos": np.full((1, a), 9, np.uint8), "neg": np.full((1, a), 9, np.uint8)}
    for missing in outs:
        ptr = {k: (None if k == missing else v) for k, v in outs.items()}
        st = lib.bod_anchor_targets(0, a, _lib.fptr(anchors), 1, _lib.iptr(ng), _lib.fptr(boxes), _lib.fptr(classes), 8, 0.5, 0.4,
                                    _lib.fptr(ptr["cls"]), _lib.fptr(ptr["box"]),
                                    None if ptr["pos"] is None else ptr["pos"].ctypes.data_as(u8),
                                    None if ptr["neg"] is None else ptr["neg"].ctypes.data_as(u8), None, None)
        assert st == _lib.BOD_ERR_INVALID_ARG
        assert b"NULL" in lib.bod_last_error(None)
    # nothing ran: the arrays that were passed still hold their fill values
    assert np.all(outs["cls"] == -7.0) and np.all(outs["box"] == -7.0) and np.all(outs["pos"] == 9) and np.all(outs["neg"] == 9)
    st = lib.bod_anchor_targets(0, 0, _lib.fptr(anchors), 1, _lib.iptr(ng), _lib.fptr(boxes), _lib.fptr(classes), 8, 0.5, 0.4,
                                _lib.fptr(outs["cls"]), _lib.fptr(outs["box"]), outs["pos"].ctypes.data_as(u8),
                                outs["neg"].ctypes.data_as(u8), None, None)
    assert st == _lib.BOD_ERR_INVALID_ARG and b"bod_anchor_targets" in lib.bod_last_error(None)
