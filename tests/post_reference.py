"""TEST INFRASTRUCTURE shared by tests/test_gpu_post.py and tests/test_post_reference_host.py: the random head outputs the posterior
tests feed to both sides, the float64 statement of the mergeable statistics record (include/bayesod.h: cls_sum, box_moments,
cov_sum) built from those raw outputs, and the float64 IoU of the clustering stage with the reference's +1 pixel convention.
Nothing here calls the code under test."""
import numpy as np


def random_raw(rng, b, n, a, c=8, bg=3.0):
    """Head outputs shaped like a trained detector's: a few % of anchors are foreground.  cls [b,n,a,c], box [b,n,a,4],
    cov [b,n,a,10], float32.  ``bg`` is added to the last (background) logit: +3 keeps some hundred anchors of 3069, a negative
    shift keeps nearly all of them, +30 none.  (c = 8, bg = 3 draws the same stream as the generator always has.)"""
    base = rng.normal(0, 1.0, (b, 1, a, c))
    base[..., -1] += bg
    hot = rng.random((b, 1, a, 1)) < 0.04
    base[..., :-1] += hot * rng.uniform(2.0, 6.0, (b, 1, a, c - 1)) * (rng.random((b, 1, a, c - 1)) < 0.3)
    cls = (base + rng.normal(0, 0.3, (b, n, a, c))).astype(np.float32)
    box_mu = rng.normal(0, 0.5, (b, 1, a, 4))
    box = (box_mu + rng.normal(0, 0.15, (b, n, a, 4))).astype(np.float32)
    cov = (rng.normal(0, 0.4, (b, 1, a, 10)) + rng.normal(0, 0.1, (b, n, a, 10))).astype(np.float32)
    return cls, box, cov


# box_moments[4 + k] = co-moment sum (i, j) of the decoded box, lower triangle row by row (include/bayesod.h); [14], [15] are padding
MOMENT_ORDER = ((0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (2, 2), (3, 0), (3, 1), (3, 2), (3, 3))


def statistics_record(cls, box, cov, anchors):
    """The statistics record of n MC samples in float64, from raw head outputs cls [b,n,a,c], box [b,n,a,4], cov [b,n,a,10] or
    None, anchors [a,4] (v,u,h,w):  cls_sum [b,a,c] = sum over the samples of softmax(cls);  box_moments [b,a,16] = mean of the
    decoded boxes (4), then the co-moment sums  sum_n (x_i - mean_i)(x_j - mean_j)  in MOMENT_ORDER (10), then 2 zeros;
    cov_sum [b,a,10] = sum of the covariance parameters.  Written sample by sample, on purpose not through oracle.bayes_od: the
    host test compares the two."""
    cls = np.asarray(cls, np.float64)
    box = np.asarray(box, np.float64)
    anc = np.asarray(anchors, np.float64)
    b, n, a, c = cls.shape
    cls_sum = np.zeros((b, a, c))
    decoded = np.zeros((n, b, a, 4))
    for s in range(n):
        z = cls[:, s] - cls[:, s].max(axis=-1, keepdims=True)
        e = np.exp(z)
        cls_sum += e / e.sum(axis=-1, keepdims=True)
        t = box[:, s]
        decoded[s, ..., 0] = anc[:, 2] * t[..., 0] / 10.0 + anc[:, 0]
        decoded[s, ..., 1] = anc[:, 3] * t[..., 1] / 10.0 + anc[:, 1]
        decoded[s, ..., 2] = anc[:, 2] * np.minimum(np.maximum(np.exp(t[..., 2] / 5.0), 1e-4), 1e4)
        decoded[s, ..., 3] = anc[:, 3] * np.minimum(np.maximum(np.exp(t[..., 3] / 5.0), 1e-4), 1e4)
    mean = decoded.sum(axis=0) / n
    box_moments = np.zeros((b, a, 16))
    box_moments[..., :4] = mean
    for s in range(n):
        d = decoded[s] - mean
        for k, (i, j) in enumerate(MOMENT_ORDER):
            box_moments[..., 4 + k] += d[..., i] * d[..., j]
    cov_sum = None if cov is None else np.asarray(cov, np.float64).sum(axis=1)
    return cls_sum, box_moments, cov_sum


def iou_plus1(corners):
    """[m,m] float64 IoU of float32-valued corners (y1,x1,y2,x2) as the reference's bbox_iou_vuvu states it: intersection sides
    (max - min + 1), areas (x1 - x2 + 1)(y1 - y2 + 1), union + 1e-5."""
    c = np.asarray(corners, np.float64)
    y1, x1, y2, x2 = (c[:, i:i + 1] for i in range(4))
    inter = np.maximum(np.minimum(x2, x2.T) - np.maximum(x1, x1.T) + 1.0, 0.0) * \
        np.maximum(np.minimum(y2, y2.T) - np.maximum(y1, y1.T) + 1.0, 0.0)
    area = (x1 - x2 + 1.0) * (y1 - y2 + 1.0)
    return inter / ((area + area.T) - inter + 0.00001)
