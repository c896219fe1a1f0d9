"""CPU: the pieces of the device PDQ path that run on the host (bayes_od_rc_amd/prob_detection_quality.py): the mask-free
``frame_boxes`` agrees with ``frame_instances`` field by field (NumPy slice edge cases included), the split of
``image_quality`` into losses and qualities-from-losses reproduces the pre-split results bit for bit, the device path
refuses what it cannot evaluate, and without a GPU it fails loudly instead of falling back."""
import json
import os

import numpy as np
import pytest

from bayes_od_rc_amd import offline_eval, prob_detection_quality as pdq

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pdq.npz"))
SHAPE = tuple(int(v) for v in G["img_shape"])


def _golden_image(k):
    gts = []
    for b, l in zip(G["img%d_gt_boxes" % k], G["img%d_gt_labels" % k]):
        m = np.zeros(SHAPE, dtype=bool)
        m[b[1]:b[3], b[0]:b[2]] = True
        gts.append(pdq.GroundTruthInstance(m, int(l), 0, 0, bounding_box=np.array(b)))
    dets = [pdq.PBoxDetInst(G["pbox_probs"][i], G["pbox_boxes"][i], [G["pbox_covs"][i][0], G["pbox_covs"][i][1]])
            for i in G["img%d_det_idx" % k]]
    return gts, dets


# image_quality of the golden images before it was split into losses and qualities (float.hex of overall, spatial, label)
PRE_SPLIT = [
    (('0x1.5587f401bde56p+0', '0x1.8c368acc118f0p+0', '0x1.99cdfce192ec0p+0'), (2, 2, 0)),
    (('0x1.192a9c0000000p-1', '0x1.6cf0bc0000000p-1', '0x1.b13f180000000p-2'), (1, 0, 1)),
    (('0x0.0p+0', '0x0.0p+0', '0x0.0p+0'), (0, 2, 0)),
    (('0x0.0p+0', '0x0.0p+0', '0x0.0p+0'), (0, 0, 1)),
    (('0x1.92360a4496ba3p-4', '0x1.b3789623f8f6ep-2', '0x1.737dcf0a764e0p-6'), (0, 1, 1)),
]


def test_losses_then_qualities_reproduce_image_quality_bit_for_bit():
    for k, (want_q, want_n) in enumerate(PRE_SPLIT):
        gts, dets = _golden_image(k)
        r = pdq.image_quality(gts, dets)
        assert tuple(float(r[x]).hex() for x in ('overall', 'spatial', 'label')) == want_q, k
        assert (r['TP'], r['FP'], r['FN']) == want_n, k
        if gts and dets:
            fg, bg, dbg, heat = pdq.pair_losses(gts, dets)
            labels, n_fg = pdq._gt_arrays(gts)
            r2 = pdq.image_quality_from_losses(labels, n_fg, [pdq.gt_counts_for_pdq(g) for g in gts], dets, fg, bg, dbg)
            assert tuple(float(r2[x]).hex() for x in ('overall', 'spatial', 'label')) == want_q, k
            overall, spatial, label, heat2, _ = pdq.pair_qualities(gts, dets)
            np.testing.assert_array_equal(heat, heat2)
            # the false-positive numerator of every detection, as the pre-split code summed it for the false positives
            for c in range(len(dets)):
                maps = np.array([heat[:, :, c]])
                assert np.sum(pdq._log(1 - maps) * (maps > 0), axis=(1, 2))[0] == dbg[c]


def _frame_inputs(rng, n_gt, n_det, h, w):
    boxes = np.stack([rng.uniform(-40, w + 40, n_gt), rng.uniform(-40, h + 40, n_gt),
                      rng.uniform(-40, w + 40, n_gt), rng.uniform(-40, h + 40, n_gt)], axis=1)
    boxes[0] = [-30.0, -12.0, 25.0, 18.0]           # negative start: NumPy wraps it
    boxes[1] = [50.0, 40.0, 20.0, 10.0]             # stop before start: empty
    boxes[2] = [w - 20.0, h - 15.0, w + 300.0, h + 300.0]     # runs off the bottom-right edge
    onehot = np.eye(4, dtype=np.float32)[rng.integers(0, 4, n_gt)]
    means = np.stack([rng.uniform(0, h, n_det), rng.uniform(0, w, n_det), rng.uniform(5, 60, n_det), rng.uniform(5, 60, n_det)], axis=1)
    a = rng.normal(0, 0.05, (n_det, 4, 4))
    covs = np.matmul(a, np.transpose(a, (0, 2, 1))) + np.eye(4)[None] * 0.01
    cats = rng.dirichlet(np.ones(8) * 0.3, n_det).astype(np.float32)
    return onehot, boxes, means, covs, cats


def _same(record, gts, dets, shape):
    boxes, labels, pixels, counted, bdets = record
    assert boxes.dtype == np.int32 and boxes.shape == (len(gts), 4)
    for k, g in enumerate(gts):
        assert list(boxes[k]) == [int(v) for v in g.bounding_box]
        assert labels[k] == g.class_label and pixels[k] == g.num_pixels
        assert bool(counted[k]) == bool(pdq.gt_counts_for_pdq(g))
    assert len(bdets) == len(dets)
    for a, b in zip(bdets, dets):
        np.testing.assert_array_equal(a.box, b.box)
        assert a.box.dtype == b.box.dtype
        np.testing.assert_array_equal(a.class_list, b.class_list)
        for ca, cb in zip(a.covs, b.covs):
            np.testing.assert_array_equal(ca, cb)
    # the device path's conversion of the instances gives the same record
    again = pdq.box_frame_from_instances(gts, dets, shape)
    np.testing.assert_array_equal(again[0], boxes)
    assert list(again[1]) == list(labels) and list(again[2]) == list(pixels) and list(again[3]) == list(counted)


def test_frame_boxes_agrees_with_frame_instances():
    shape = (60, 80)
    for seed in range(4):
        onehot, boxes, means, covs, cats = _frame_inputs(np.random.default_rng(seed), 7, 9, *shape)
        args = (onehot, boxes, means, covs, cats, shape)
        _same(pdq.frame_boxes(*args), *pdq.frame_instances(*args), shape)
        kw = dict(score_threshold=0.5, class_columns=(0, 3), gt_boxes_vuvu=True, clip_max=70)
        _same(pdq.frame_boxes(*args, **kw), *pdq.frame_instances(*args, **kw), shape)
        low = dict(score_threshold=0.2, cov_scale=3.0)
        _same(pdq.frame_boxes(*args, **low), *pdq.frame_instances(*args, **low), shape)
    # no detections, no objects
    empty = pdq.frame_boxes(np.zeros((0, 4)), np.zeros((0, 4)), np.zeros((0, 4)), np.zeros((0, 4, 4)), np.zeros((0, 8)), shape)
    assert empty[0].shape == (0, 4) and empty[1:4] == ([], [], []) and empty[4] == []


def test_device_path_refuses_what_it_cannot_evaluate():
    gts, dets = _golden_image(0)
    m = gts[0].segmentation_mask.copy()
    m[0, 0] = not m[0, 0]
    odd = pdq.GroundTruthInstance(m, 1, 0, 0, bounding_box=gts[0].bounding_box)
    with pytest.raises(ValueError, match="box-shaped"):
        pdq.box_frame_from_instances([odd], dets, SHAPE)
    with pytest.raises(ValueError, match="PBoxDetInst"):
        pdq.box_frame_from_instances(gts, [pdq.BBoxDetInst(G["pbox_probs"][0], G["bbox_box"], 0.8)], SHAPE)
    with pytest.raises(ValueError, match="integer"):
        pdq._det_arrays([pdq.PBoxDetInst(G["pbox_probs"][0], np.array([1.5, 2.0, 9.0, 9.0]), [np.eye(2), np.eye(2)])])


def test_records_grouped_by_frame_read_like_read_bdd_frame():
    recs = [{'name': 'b', 'category': 'car', 'bbox': [1, 2, 3, 4]}, {'name': 'a', 'category': 'person', 'bbox': [5, 6, 7, 8]},
            {'name': 'b', 'category': 'train', 'bbox': [0, 0, 9, 9]}, {'name': 'b', 'category': 'bus', 'bbox': [2, 2, 8, 8]}]
    by = offline_eval._records_by_frame(recs)
    for name in ('a', 'b', 'c'):
        want = offline_eval.read_bdd_frame(name, recs)
        got = offline_eval._bdd_frame_arrays(by.get(name, []))
        for x, y in zip(got, want):
            np.testing.assert_array_equal(x, y)


def test_no_gpu_means_loud_failure(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bayes-od-rc_amd", "lib",
                                       "libbayesod_hip.so")):
        g.build()
    from test_offline_eval import SHAPE as TREE_SHAPE, _tree
    root, labels, gt = _tree(tmp_path, clutter=1)
    frames = sorted(f[:-4] for f in os.listdir(os.path.join(root, 'mean')))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        offline_eval.pdq_report(gt, root, frames, TREE_SHAPE, device=0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pdq.evaluate([_golden_image(0)], device=0)
    with open(labels) as fp:
        assert json.load(fp) == gt
