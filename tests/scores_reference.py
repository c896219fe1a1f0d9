"""Shared inputs of the scoring-rule tests (test_scoring_rules_host.py, test_gpu_scores.py): seeded positive-definite
pairs, and a small prediction tree with hand-computed matching counts."""
import json
import os

import numpy as np

def pd_pairs(n, seed=7):
    """n rows (mu, Sigma, g): Sigma = (A A^T + 0.5 I) s with A standard normal and s cycling over 1e-2, 9, 1e4; mu of box
    magnitude; g = mu + a few sigma."""
    rng = np.random.default_rng(seed)
    a = rng.normal(size=(n, 4, 4))
    s = np.array([1e-2, 9.0, 1e4])[np.arange(n) % 3]
    covs = (a @ np.transpose(a, (0, 2, 1)) + 0.5 * np.eye(4)) * s[:, None, None]
    means = rng.uniform(50.0, 900.0, size=(n, 4))
    sig = np.sqrt(covs[:, np.arange(4), np.arange(4)])
    targets = means + rng.uniform(-3.0, 3.0, size=(n, 4)) * sig
    return means, covs, targets


def _vuhw(x1, y1, x2, y2):
    return [(y1 + y2) / 2.0, (x1 + x2) / 2.0, float(y2 - y1), float(x2 - x1)]


def _cat(best, score, background=None):
    """8 class parameters summing to 1: `score` on class `best`, `background` (default: half the rest) on the last."""
    rest = 1.0 - score
    bg = rest / 2.0 if background is None else background
    p = np.full(8, (rest - bg) / 6.0)
    p[best] = score
    p[7] = bg
    return p


# expected by hand (see write_tree): true positives, false positives, unmatched ground truth, singular true positives
TREE_COUNTS = {'n_tp': 5, 'n_fp': 5, 'n_fn': 2, 'n_singular': 1}
TREE_FRAMES = ['a', 'b', 'c']


def write_tree(root, parts=True):
    """3 frames, 12 detections.  Frame a: ground truth car G0, person G1, truck G2, bus G3.
         d0 on G0 (0.90 car)             true positive
         d1 on G0 (0.80 car)             false positive: G0 is taken
         d2 on G1 (0.70 rider)           true positive (class-agnostic), wrong class
         d3 far from everything (0.95)   false positive
         d4 on G2 (0.30)                 below the score threshold: dropped, G2 stays unmatched
         d5 half off G2 (0.60)           false positive (IoU < 0.5)
         d6 on G3 (0.66), Sigma = diag(0, 9, 0, 16) in (v, u, h, w): var(y1) = 0, the second pivot is exactly 0 at any scale -> singular
       Frame b: one car, no detections -> one unmatched ground truth.
       Frame c: cars G0, G1 and a 'traffic light' (not a category: ignored).
         d0 on G0 (0.85) true positive; d1 on G1 (0.75) false positive: d2 on G1 (0.90) came first, true positive;
         d3 background (best class 0.20) dropped; d4 on the traffic light (0.65) false positive.
    Returns (ground-truth records, tree directory)."""
    rng = np.random.default_rng(3)
    gt = [{'name': 'a', 'category': 'car', 'bbox': [100, 100, 200, 180]},
          {'name': 'a', 'category': 'person', 'bbox': [300, 200, 340, 300]},
          {'name': 'a', 'category': 'truck', 'bbox': [500, 100, 700, 300]},
          {'name': 'a', 'category': 'bus', 'bbox': [800, 400, 900, 500]},
          {'name': 'b', 'category': 'car', 'bbox': [10, 10, 60, 50]},
          {'name': 'c', 'category': 'car', 'bbox': [50, 60, 150, 140]},
          {'name': 'c', 'category': 'car', 'bbox': [400, 300, 520, 380]},
          {'name': 'c', 'category': 'traffic light', 'bbox': [600, 20, 620, 60]}]
    frames = {
        'a': ([_vuhw(103, 98, 204, 183), _vuhw(95, 104, 197, 176), _vuhw(302, 203, 338, 296), _vuhw(1000, 600, 1100, 650),
               _vuhw(500, 100, 700, 300), _vuhw(600, 100, 800, 300), _vuhw(802, 403, 897, 499)],
              [_cat(0, 0.90), _cat(0, 0.80), _cat(4, 0.70), _cat(1, 0.95), _cat(1, 0.30), _cat(1, 0.60), _cat(2, 0.66)]),
        'b': ([], []),
        'c': ([_vuhw(52, 58, 149, 143), _vuhw(403, 297, 515, 384), _vuhw(398, 302, 522, 377), _vuhw(200, 200, 260, 260),
               _vuhw(600, 20, 620, 60)],
              [_cat(0, 0.85), _cat(0, 0.75), _cat(0, 0.90), _cat(3, 0.20, background=0.7), _cat(5, 0.65)]),
    }
    dirs = ['mean', 'cov', 'cat_param'] + (['cov_epistemic', 'cov_aleatoric', 'cov_prior'] if parts else [])
    for d in dirs:
        os.makedirs(os.path.join(root, d), exist_ok=True)
    for name, (means, cats) in frames.items():
        k = len(means)
        a = rng.normal(size=(k, 4, 4))
        cov = (a @ np.transpose(a, (0, 2, 1)) + 0.5 * np.eye(4)) * 6.0
        if name == 'a':
            cov[6] = np.diag([0.0, 9.0, 0.0, 16.0])
        np.save(os.path.join(root, 'mean', name + '.npy'), np.array(means, np.float32).reshape(k, 4))
        np.save(os.path.join(root, 'cov', name + '.npy'), cov.astype(np.float32).reshape(k, 4, 4))
        np.save(os.path.join(root, 'cat_param', name + '.npy'), np.array(cats, np.float32).reshape(k, 8))
        if parts:                     # the parts are fixed shares of cov
            c32 = cov.astype(np.float32).reshape(k, 4, 4)
            for d, share in (('cov_epistemic', 0.25), ('cov_aleatoric', 0.25), ('cov_prior', 0.5)):
                np.save(os.path.join(root, d, name + '.npy'), c32 * np.float32(share))
    with open(os.path.join(root, 'labels.json'), 'w') as fp:
        json.dump(gt, fp)
    return gt, root
