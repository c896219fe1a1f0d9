"""CPU: the test infrastructure of tests/post_reference.py against the oracle -- the statistics record the GPU posterior tests feed
to set_statistics must say what oracle.bayes_od computes from the same raw outputs, and the +1-convention IoU must be
oracle.geometry's."""
import numpy as np
import pytest

import post_reference as pr
from conftest import ANCHOR_CFG
from oracle import bayes_od, geometry


def _anchors():
    return geometry.generate_all_anchors((128, 128, 3), ANCHOR_CFG["layers"], ANCHOR_CFG["aspect_ratios"], ANCHOR_CFG["scales"])


@pytest.mark.parametrize("c,n,bg", [(8, 5, 3.0), (4, 2, -20.0), (4, 7, 30.0)])
def test_statistics_record_is_the_oracles_mean_and_covariance(c, n, bg):
    anchors = _anchors()
    a = anchors.shape[0]
    assert a == 3069
    rng = np.random.default_rng(100 + c + n)
    cls, box, cov = pr.random_raw(rng, 2, n, a, c=c, bg=bg)
    box[0, :, 5, 2] = 50.0          # both clamps of the decode
    box[1, :, 6, 3] = -50.0
    cls_sum, moments, cov_sum = pr.statistics_record(cls, box, cov, anchors)
    assert cls_sum.dtype == moments.dtype == cov_sum.dtype == np.float64
    assert cls_sum.shape == (2, a, c) and moments.shape == (2, a, 16) and cov_sum.shape == (2, a, 10)
    assert np.all(moments[..., 14:] == 0)
    for img in range(2):
        probs = bayes_od.softmax(cls[img].astype(np.float64))
        assert np.allclose(cls_sum[img] / n, probs.mean(axis=0), rtol=1e-13, atol=0)
        boxes = geometry.box_from_anchor_and_target(anchors[None].astype(np.float64), box[img].astype(np.float64))
        mu, cov_epi = bayes_od.mean_covariance(boxes)
        assert np.allclose(moments[img, :, :4], mu, rtol=1e-13, atol=0)
        got = np.zeros((a, 4, 4))
        for k, (i, j) in enumerate(pr.MOMENT_ORDER):
            got[:, i, j] = got[:, j, i] = moments[img, :, 4 + k] / (n - 1.0)
        scale = np.abs(cov_epi).reshape(a, -1).max(axis=1)[:, None, None]
        assert np.all(np.abs(got - cov_epi) <= 1e-12 * scale)
        assert np.allclose(cov_sum[img] / n, cov[img].astype(np.float64).mean(axis=0), rtol=1e-13, atol=1e-15)
    assert moments[0, 5, 2] == pytest.approx(anchors[5, 2] * 1e4) and moments[1, 6, 3] == pytest.approx(anchors[6, 3] * 1e-4)
    assert pr.statistics_record(cls, box, None, anchors)[2] is None


def test_random_raw_default_stream_is_unchanged():
    """c = 8, bg = +3 is the generator the posterior tests have always used (their expected kept counts depend on it)."""
    rng = np.random.default_rng(21)
    cls, box, cov = pr.random_raw(rng, 2, 5, 3069)
    rng = np.random.default_rng(21)
    base = rng.normal(0, 1.0, (2, 1, 3069, 8))
    base[..., -1] += 3.0
    hot = rng.random((2, 1, 3069, 1)) < 0.04
    base[..., :-1] += hot * rng.uniform(2.0, 6.0, (2, 1, 3069, 7)) * (rng.random((2, 1, 3069, 7)) < 0.3)
    assert np.array_equal(cls, (base + rng.normal(0, 0.3, (2, 5, 3069, 8))).astype(np.float32))
    assert cls.dtype == box.dtype == cov.dtype == np.float32 and box.shape == (2, 5, 3069, 4) and cov.shape == (2, 5, 3069, 10)


def test_iou_plus1_is_the_oracles_formula():
    rng = np.random.default_rng(2)
    tl = rng.uniform(0, 80, (50, 2))
    corners = np.concatenate([tl, tl + rng.uniform(2, 40, (50, 2))], axis=1).astype(np.float32)
    corners[7] = corners[3]
    ref = geometry.bbox_iou_vuvu(corners.astype(np.float64), corners.astype(np.float64))
    got = pr.iou_plus1(corners)
    assert got.dtype == np.float64 and np.allclose(got, ref, rtol=1e-14, atol=0)
    assert got[7, 3] == got[3, 3] and np.array_equal(got, got.T)
