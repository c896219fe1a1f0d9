"""Proper scoring rules and calibration of the detector's predictive distributions.

For a true-positive detection the box posterior is a 4-dimensional Gaussian N(mu, Sigma) over the corners (x1, y1, x2, y2)
and the matched ground-truth box g is one observation of it.  Per pair (``score_pairs_np``, device twin
``engine.score_pairs`` / score_kernels.hip), with L the lower Cholesky factor of Sigma:

    nll    = 0.5 (4 ln 2pi + ln det Sigma + m2)             m2 = |L^-1 (g - mu)|^2   (squared Mahalanobis distance)
    ES     = (1/M) sum_{i<M} |z_i - g| - 1/(2(M-1)) sum_{i<M-1} |z_i - z_{i+1}|,   z_i = mu + L n_i   (energy score)
    PIT_k  = Phi((g_k - mu_k) / sqrt(Sigma_kk)) = 0.5 erfc(-(g_k - mu_k) / sqrt(2 Sigma_kk))
    ln det Sigma = 2 sum ln L_kk

The normals n_i are DEFINED by the project's Philox contract: sample i of the row with 64-bit id r is one call
philox4x32_10(i, r & 0xffffffff, SCORE_TAG, r >> 32, seed_lo, seed_hi) -> (x, y, z, w), u(t) = (t + 0.5) 2^-32, and two
Box-Muller pairs n0, n1 = sqrt(-2 ln u(x)) (cos, sin)(2 pi u(y)), n2, n3 from (z, w).  A row's result depends on its id
alone, so host and device, one call or many, give the same numbers.

``scores_report`` matches detections to ground truth (``match_frame``: the greedy rule of evaluation_utils_2d._match),
scores the pairs and summarises them; ``offline_eval scores`` is its command line.  Host NumPy, float64.
"""
import math
import os

import numpy as np
from scipy.special import erfc

from .offline_eval import BDD_CATEGORIES, _load, _records_by_frame
from .prob_detection_quality import _VUHW_TO_CORNERS

SCORE_TAG = 0x005C04E5
MIN_SAMPLES, MAX_SAMPLES = 2, 65536
_CHUNK_SAMPLES = 1 << 20          # samples in flight per chunk of rows: the Philox words and normals stay around 200 MB

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK32, _S32 = np.uint64(0xFFFFFFFF), np.uint64(32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (csrc/philox.h): counter words broadcast against each other, scalar key; four uint32 arrays."""
    c0, c1, c2, c3 = np.broadcast_arrays(*(np.asarray(c, dtype=np.uint64) & _MASK32 for c in (c0, c1, c2, c3)))
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ np.uint64(k0), p1 & _MASK32, (p0 >> _S32) ^ c3 ^ np.uint64(k1), p0 & _MASK32
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def score_normals(row_ids, num_samples, seed):
    """The contract's standard normals [len(row_ids), num_samples, 4] (float64)."""
    r = np.asarray(row_ids, dtype=np.uint64).reshape(-1, 1)
    i = np.arange(num_samples, dtype=np.uint64)[None, :]
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    x, y, z, w = philox4x32_10(i, r & _MASK32, np.uint64(SCORE_TAG), r >> _S32, seed & 0xFFFFFFFF, seed >> 32)
    u = [(t.astype(np.float64) + 0.5) * 2.0 ** -32 for t in (x, y, z, w)]
    r0, r1 = np.sqrt(-2.0 * np.log(u[0])), np.sqrt(-2.0 * np.log(u[2]))
    a0, a1 = (2.0 * math.pi) * u[1], (2.0 * math.pi) * u[3]
    return np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1), r1 * np.sin(a1)], axis=-1)


def _cholesky_lower(covs):
    """Cholesky-Banachiewicz on the lower triangles of covs [n,4,4]: (L [n,4,4], ok [n]).  A pivot <= 0 or non-finite
    clears ``ok``; that row's factor is meaningless."""
    n = covs.shape[0]
    L = np.zeros((n, 4, 4), np.float64)
    ok = np.ones(n, bool)
    with np.errstate(all='ignore'):
        for k in range(4):
            for j in range(k):
                s = covs[:, k, j].copy()
                for p in range(j):
                    s -= L[:, k, p] * L[:, j, p]
                L[:, k, j] = s / L[:, j, j]
            d = covs[:, k, k].copy()
            for p in range(k):
                d -= L[:, k, p] * L[:, k, p]
            good = (d > 0.0) & np.isfinite(d)
            ok &= good
            L[:, k, k] = np.sqrt(np.where(good, d, 1.0))
    return L, ok


def score_pairs_np(means, covs, targets, num_samples=1000, seed=0, first_row_id=0):
    """Host statement of ``bod_score_pairs``: (out [n,8] = nll, m2, energy score, PIT x4, ln det; status [n] int32 with
    2 = non-finite input (mean, target, lower triangle), 1 = not positive definite, 0 = scored).  Rows with status != 0 are
    NaN.  Row i uses the id ``first_row_id + i``."""
    means = np.asarray(means, dtype=np.float64).reshape(-1, 4)
    ids = np.uint64(int(first_row_id) & 0xFFFFFFFFFFFFFFFF) + np.arange(means.shape[0], dtype=np.uint64)     # (wraps modulo 2^64 like the device's)
    return score_rows_np(means, covs, targets, ids, num_samples, seed)


def score_rows_np(means, covs, targets, row_ids, num_samples=1000, seed=0):
    """``score_pairs_np`` with an explicit 64-bit id per row."""
    means = np.asarray(means, dtype=np.float64).reshape(-1, 4)
    covs = np.asarray(covs, dtype=np.float64).reshape(-1, 4, 4)
    targets = np.asarray(targets, dtype=np.float64).reshape(-1, 4)
    row_ids = np.asarray(row_ids, dtype=np.uint64).reshape(-1)
    n = means.shape[0]
    if covs.shape[0] != n or targets.shape[0] != n or row_ids.shape[0] != n:
        raise ValueError("means, covs, targets and ids must have one row per pair")
    num_samples = int(num_samples)
    if not MIN_SAMPLES <= num_samples <= MAX_SAMPLES:
        raise ValueError("num_samples %d outside [%d, %d]" % (num_samples, MIN_SAMPLES, MAX_SAMPLES))
    out = np.full((n, 8), np.nan, np.float64)
    status = np.zeros(n, np.int32)
    if n == 0:
        return out, status
    tril = np.tril(np.ones((4, 4), bool))
    finite = np.isfinite(means).all(1) & np.isfinite(targets).all(1) & np.isfinite(covs[:, tril]).all(1)
    status[~finite] = 2
    L, pd = _cholesky_lower(np.where(finite[:, None, None], covs, np.eye(4)))
    status[finite & ~pd] = 1
    rows = np.nonzero(status == 0)[0]
    if not rows.size:
        return out, status
    mu, g, Lr, ids = means[rows], targets[rows], L[rows], row_ids[rows]
    diag = Lr[:, np.arange(4), np.arange(4)]
    logdet = 2.0 * np.sum(np.log(diag), axis=1)
    y = np.zeros_like(mu)
    for k in range(4):                                    # forward substitution L y = g - mu
        s = g[:, k] - mu[:, k]
        for p in range(k):
            s = s - Lr[:, k, p] * y[:, p]
        y[:, k] = s / Lr[:, k, k]
    m2 = np.sum(y * y, axis=1)
    out[rows, 0] = 0.5 * (4.0 * math.log(2.0 * math.pi) + logdet + m2)
    out[rows, 1] = m2
    var = covs[rows][:, np.arange(4), np.arange(4)]
    out[rows[:, None], np.arange(3, 7)[None, :]] = 0.5 * erfc(-(g - mu) / np.sqrt(2.0 * var))
    out[rows, 7] = logdet
    step = max(1, _CHUNK_SAMPLES // num_samples)
    for lo in range(0, rows.size, step):
        sl = slice(lo, lo + step)
        z = mu[sl, None, :] + np.einsum('rkp,rip->rik', Lr[sl], score_normals(ids[sl], num_samples, seed))
        a = np.sqrt(np.sum((z - g[sl, None, :]) ** 2, axis=-1))
        b = np.sqrt(np.sum((z[:, 1:] - z[:, :-1]) ** 2, axis=-1))
        out[rows[sl], 2] = a.sum(axis=1) / num_samples - b.sum(axis=1) / (2.0 * (num_samples - 1))
    return out, status


def match_frame(gt_boxes_xyxy, det_boxes_xyxy, det_order, iou_threshold=0.5):
    """The greedy rule of evaluation_utils_2d._match on one frame, class-agnostic: in ``det_order`` every detection claims
    the ground-truth box it overlaps most (+1 pixel IoU, first of equals); it is a true positive if that IoU > threshold
    and the box is not yet taken, else a false positive.  Returns (pairs [(detection, ground truth)], false positives,
    unmatched ground truth), detections in the order given."""
    gt = np.asarray(gt_boxes_xyxy, dtype=np.float64).reshape(-1, 4)
    det = np.asarray(det_boxes_xyxy, dtype=np.float64).reshape(-1, 4)
    taken = np.zeros(len(gt), bool)
    pairs, fps = [], []
    for d in det_order:
        d = int(d)
        box = det[d]
        ovmax, jmax = -np.inf, -1
        if len(gt):
            iw = np.maximum(np.minimum(gt[:, 2], box[2]) - np.maximum(gt[:, 0], box[0]) + 1.0, 0.0)
            ih = np.maximum(np.minimum(gt[:, 3], box[3]) - np.maximum(gt[:, 1], box[1]) + 1.0, 0.0)
            inters = iw * ih
            uni = (box[2] - box[0] + 1.0) * (box[3] - box[1] + 1.0) + (gt[:, 2] - gt[:, 0] + 1.0) * (gt[:, 3] - gt[:, 1] + 1.0) - inters
            overlaps = inters / uni
            ovmax, jmax = np.max(overlaps), int(np.argmax(overlaps))
        if ovmax > iou_threshold and not taken[jmax]:
            taken[jmax] = True
            pairs.append((d, jmax))
        else:
            fps.append(d)
    return pairs, fps, [int(j) for j in np.nonzero(~taken)[0]]


_REGRESSION_KEYS = ('mean_nll', 'median_nll', 'mean_energy_score', 'mean_mahalanobis2', 'calibration_error', 'fitted_cov_scale',
                    'nll_at_fitted_scale')


def regression_summary(out, status):
    """The regression block of the report from ``score_pairs`` results; rows with status != 0 are counted and left out."""
    good = np.asarray(status) == 0
    o = np.asarray(out, np.float64)[good]
    block = {'n_singular': int(np.sum(~good))}
    if not o.shape[0]:
        block.update({k: None for k in _REGRESSION_KEYS})
        return block
    nll, m2, es, pit, logdet = o[:, 0], o[:, 1], o[:, 2], o[:, 3:7], o[:, 7]
    qs = np.arange(1, 10) / 10.0
    share = np.mean(pit[:, :, None] <= qs[None, None, :], axis=0)            # [4 coordinates, 9 levels]
    s_fit = float(np.mean(m2) / 4.0)
    block.update({'mean_nll': float(np.mean(nll)), 'median_nll': float(np.median(nll)), 'mean_energy_score': float(np.mean(es)),
                  'mean_mahalanobis2': float(np.mean(m2)), 'calibration_error': float(np.mean(np.abs(share - qs[None, :]))),
                  'fitted_cov_scale': s_fit,
                  # d/ds mean 0.5 (4 ln s + m2 / s) = 0  at  s = mean(m2) / 4
                  'nll_at_fitted_scale': (float(np.mean(0.5 * (4.0 * math.log(2.0 * math.pi) + logdet + 4.0 * math.log(s_fit) + m2 / s_fit)))
                                          if s_fit > 0 else None)})
    return block


def _score(means, covs, targets, ids, num_samples, seed, device):
    """The report's pairs with their ids (frame * 2^16 + detection).  On the host every row carries its id.  bod_score_pairs
    numbers the rows of a call consecutively, so the device gets one call per frame: the frame's detection indices from the
    lowest to the highest paired one form a block of consecutive ids; an index without a pair holds a copy of the block's
    first pair and its result is dropped."""
    ids = np.asarray(ids, dtype=np.int64)
    if device is None:
        return score_rows_np(means, covs, targets, ids, num_samples, seed)
    from . import engine
    out = np.full((len(ids), 8), np.nan, np.float64)
    status = np.zeros(len(ids), np.int32)
    order = np.argsort(ids, kind='stable')
    cuts = np.nonzero(np.diff(ids[order] >> 16))[0] + 1
    for idx in np.split(order, cuts) if len(ids) else []:
        base = int(ids[idx[0]])
        slot = ids[idx] - base
        src = np.full(int(slot[-1]) + 1, idx[0])
        src[slot] = idx
        o, s = engine.score_pairs(means[src], covs[src], targets[src], num_samples, seed, base, device=device)
        out[idx], status[idx] = o[slot], s[slot]
    return out, status


def scores_report(gt_records, tree, frames, categories=BDD_CATEGORIES, score_threshold=0.5445, iou_threshold=0.5, cov_scale=1.0,
                  num_samples=1000, seed=0, device=None, parts=False):
    """Scores the prediction tree's distributions against BDD-format ground-truth records.

    Detections: the rows of mean/ cov/ cat_param/ whose best non-background score (the last column of cat_param is the
    background) reaches ``score_threshold``, taken in descending order of that score (ties: file order) by ``match_frame``.
    Boxes and covariances move to corners with T mu and T Sigma T^T * cov_scale.  A pair's row id is (frame index in
    ``frames``) * 2^16 + detection index, so the report does not depend on how the rows reach the scorer.  ``device`` None
    = score_pairs_np, an integer = bod_score_pairs on that GPU.  ``parts``: repeat the regression block with the matrices
    of cov_epistemic/, cov_aleatoric/ and their sum in place of cov/ (trees written with the covariance parts)."""
    categories = tuple(categories)
    by_frame = _records_by_frame(gt_records)
    part_dirs = ('cov_epistemic', 'cov_aleatoric', 'cov_prior')
    with_parts = bool(parts) and all(os.path.isdir(os.path.join(tree, d)) for d in part_dirs)
    T = _VUHW_TO_CORNERS
    mus, covs, gs, ids = [], [], [], []
    part_covs = {'epistemic': [], 'aleatoric': []}
    tp_probs, tp_labels, fp_bg = [], [], []
    ece_conf, ece_hit = [], []
    n_fn = 0
    for fi, frame in enumerate(frames):
        rows = [g for g in by_frame.get(frame, []) if g['category'] in categories]
        gt_boxes = np.array([g['bbox'] for g in rows], np.float64).reshape(-1, 4)
        gt_labels = [categories.index(g['category']) for g in rows]
        means = np.asarray(_load(tree, 'mean', frame), np.float64).reshape(-1, 4)
        if not means.shape[0]:
            n_fn += len(rows)
            continue
        if means.shape[0] > 1 << 16:
            raise ValueError("frame %s: more than 65536 detections" % frame)
        cats = np.asarray(_load(tree, 'cat_param', frame), np.float64).reshape(means.shape[0], -1)
        probs = cats / np.sum(cats, axis=1, keepdims=True)
        best = np.max(cats[:, :-1], axis=1)
        kept = np.nonzero(best >= score_threshold)[0]
        order = kept[np.argsort(-best[kept], kind='stable')]
        boxes = means @ T.T
        pairs, fps, fns = match_frame(gt_boxes, boxes, order, iou_threshold)
        n_fn += len(fns)
        if pairs:
            d_idx = np.array([d for d, _ in pairs])
            cov = np.asarray(_load(tree, 'cov', frame), np.float64).reshape(-1, 4, 4)
            mus.append(boxes[d_idx])
            covs.append(T @ (cov[d_idx] * cov_scale) @ T.T)
            gs.append(gt_boxes[[j for _, j in pairs]])
            ids.extend(fi * (1 << 16) + int(d) for d in d_idx)
            if with_parts:
                for key in part_covs:
                    pc = np.asarray(_load(tree, 'cov_' + key, frame), np.float64).reshape(-1, 4, 4)
                    part_covs[key].append(T @ (pc[d_idx] * cov_scale) @ T.T)
        for d, j in pairs:
            tp_probs.append(probs[d])
            tp_labels.append(gt_labels[j])
            ece_conf.append(best[d])
            ece_hit.append(float(int(np.argmax(cats[d])) == gt_labels[j]))
        for d in fps:
            fp_bg.append(probs[d, -1])
            ece_conf.append(best[d])
            ece_hit.append(0.0)
    n_tp = len(ids)

    def cat(blocks, shape):
        return np.concatenate(blocks) if blocks else np.zeros((0,) + shape, np.float64)

    mu_a, cov_a, g_a = cat(mus, (4,)), cat(covs, (4, 4)), cat(gs, (4,))
    report = {'n_tp': n_tp, 'n_fp': len(fp_bg), 'n_fn': int(n_fn)}
    report.update(regression_summary(*_score(mu_a, cov_a, g_a, ids, num_samples, seed, device)))
    tiny = np.finfo(np.float64).tiny
    if n_tp:
        p = np.array(tp_probs)
        onehot = np.zeros_like(p)
        onehot[np.arange(n_tp), tp_labels] = 1.0
        report['cls_nll'] = float(np.mean(-np.log(np.maximum(p[np.arange(n_tp), tp_labels], tiny))))
        report['brier'] = float(np.mean(np.sum((p - onehot) ** 2, axis=1)))
    else:
        report['cls_nll'] = report['brier'] = None
    report['fp_nll'] = float(np.mean(-np.log(np.maximum(np.array(fp_bg), tiny)))) if fp_bg else None
    if ece_conf:
        conf, hit = np.array(ece_conf), np.array(ece_hit)
        bins = np.minimum((conf * 10.0).astype(np.int64), 9)               # 10 equal bins of [0, 1]; 1.0 belongs to the last
        ece = 0.0
        for b in range(10):
            m = bins == b
            if m.any():
                ece += np.sum(m) / conf.size * abs(np.mean(hit[m]) - np.mean(conf[m]))
        report['ece'] = float(ece)
    else:
        report['ece'] = None
    if with_parts:
        epi, ale = cat(part_covs['epistemic'], (4, 4)), cat(part_covs['aleatoric'], (4, 4))
        report['parts'] = {name: regression_summary(*_score(mu_a, c, g_a, ids, num_samples, seed, device))
                           for name, c in (('epistemic', epi), ('aleatoric', ale), ('epistemic+aleatoric', epi + ale))}
    return report
