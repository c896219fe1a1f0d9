"""The cluster merge methods of include/bayesod.h (bod_set_merge_method) restated in NumPy float64, the bounds a
float32 kernel is held to, and the clustered posteriors the tests feed both sides.

Membership: rows whose affinity to centre k is > thr (the IoU of the means, or the caller's matrix).  With n members, c the
centre's row and d_i = mu_i - mu_c:

  centre    mean = mu_c, cov = within = Sigma_c, between = 0, counts = counts_c, scores = counts_c / sum(counts_c)
  mixture   dbar = (1/n) sum d_i, mean = mu_c + dbar, within = (1/n) sum Sigma_i, between = (1/n) sum d_i d_i^T - dbar dbar^T,
            cov = within + between, scores = (1/n) sum counts_i / sum(counts_i), counts = (1/n) sum counts_i
  n == 0    the centre's row as `centre` gives it, members = 0
"""
import numpy as np

import post_reference

EPS = 64.0 * 2.0 ** -24          # at most ceil(n / 256) serial adds + 8 tree levels + the products and the final subtraction: <= 16 roundings, times 4


def iou_affinity(means):
    """[m,m] float64 IoU of the corners the device derives from float32 means (v,u,h,w)."""
    from oracle import geometry
    return post_reference.iou_plus1(geometry.vuhw_to_vuvu(np.asarray(means, np.float32)))


def clustered_posteriors(rng, sizes, c, singles=0, distractors=2):
    """Boxes in clusters of the given sizes on a wide canvas (cell k holds cluster k: members jittered by a pixel around the
    cluster's first box, IoU ~ 0.9; `distractors` boxes per cluster shifted by 0.45 of its height, IoU ~ 0.4), plus `singles`
    boxes alone in their cells; all shuffled, so a cluster's members fall on the threads of the block in no order.
    Returns counts [m,c], means [m,4] (v,u,h,w), covs [m,4,4] (exactly symmetric), float32, and each cluster's first box."""
    boxes, first = [], []
    for k, size in enumerate(list(sizes) + [1] * singles):
        base = np.array([80.0 + 150.0 * (k // 40), 80.0 + 150.0 * (k % 40), rng.uniform(30, 60), rng.uniform(30, 60)])
        first.append(len(boxes))
        boxes.append(base)
        for _ in range(size - 1):
            boxes.append(np.concatenate([base[:2] + rng.normal(0, 1.0, 2), base[2:] * np.exp(rng.normal(0, 0.02, 2))]))
        for _ in range(distractors if k < len(sizes) else 0):
            boxes.append(base + np.array([0.45 * base[2] * rng.choice([-1.0, 1.0]), 0.0, 0.0, 0.0]))
    m = len(boxes)
    perm = rng.permutation(m)
    inv = np.empty(m, np.int64)
    inv[perm] = np.arange(m)
    means = np.stack(boxes)[perm].astype(np.float32)
    a = rng.normal(size=(m, 4, 4))
    covs = (a @ a.transpose(0, 2, 1) + 2.0 * np.eye(4)).astype(np.float32)
    covs = np.tril(covs) + np.tril(covs, -1).transpose(0, 2, 1)          # the lower triangle, mirrored
    cnt = rng.integers(0, 6, (m, c)) + rng.uniform(0.1, 1.0, (m, c))
    return cnt.astype(np.float32), means, covs, inv[np.asarray(first)][:len(sizes)].astype(np.int32)


def member_columns(means, centres, affinity=None, thr=0.5, guard=1e-4):
    """[m,k] bool membership; asserts that no affinity lies within `guard` of the threshold (a float32 kernel must agree on it).
    1e-4 for posteriors a test builds; a posterior that came out of the network is taken as it is, and the float32 IoU of boxes
    of tens of pixels is within 1e-6 of the float64 one."""
    if affinity is None:
        affinity = iou_affinity(means)
    cols = np.asarray(affinity, np.float64)[:, np.asarray(centres, np.int64)]
    assert cols.size == 0 or np.abs(cols - thr).min() > guard
    return cols > thr


def merge_reference(counts, means, covs, centres, affinity=None, thr=0.5, method="mixture", guard=1e-4):
    """float64 on the float32-valued inputs.  Returns a dict: scores [k,c], means [k,4], covs [k,4,4], counts [k,c], within
    [k,4,4], between [k,4,4], members [k], and `bound`: the same keys -> the absolute error a float32 kernel may show, entry by
    entry (mixture: EPS times the mean magnitude of the terms that enter the entry; where n == 0 or the method is 'centre' the
    result is a copy or one quotient: 0 for the copies, 2^-23 relative of the float32 quotient for the scores)."""
    assert method in ("centre", "mixture")
    counts = np.asarray(counts, np.float64)
    means = np.asarray(means, np.float64).reshape(-1, 4)
    covs = np.asarray(covs, np.float64).reshape(-1, 4, 4)
    centres = np.asarray(centres)
    member = member_columns(means.astype(np.float32), centres, affinity, thr, guard)
    k, c = len(centres), counts.shape[1]
    out = {"scores": np.zeros((k, c)), "means": np.zeros((k, 4)), "covs": np.zeros((k, 4, 4)), "counts": np.zeros((k, c)),
           "within": np.zeros((k, 4, 4)), "between": np.zeros((k, 4, 4)), "members": member.sum(axis=0).astype(np.int32)}
    bound = {key: np.zeros_like(out[key]) for key in ("scores", "means", "covs", "counts", "within", "between")}
    for j, ctr in enumerate(centres):
        idx = np.nonzero(member[:, j])[0]
        n = len(idx)
        if method == "centre" or n == 0:
            out["means"][j], out["covs"][j], out["within"][j], out["counts"][j] = means[ctr], covs[ctr], covs[ctr], counts[ctr]
            out["scores"][j] = counts[ctr] / counts[ctr].sum()
            # the rule holds the kernel to 2^-23 relative of the FLOAT32 quotient (its sum taken for j ascending), which itself
            # sits a few roundings from the float64 one stated here
            q32 = centre_scores_f32(counts[ctr]).astype(np.float64)
            bound["scores"][j] = np.abs(q32 - out["scores"][j]) + 2.0 ** -23 * q32
            continue
        d = means[idx] - means[ctr]
        dbar = d.mean(axis=0)
        dd = d[:, :, None] * d[:, None, :]
        within = covs[idx].mean(axis=0)
        between = dd.mean(axis=0) - np.outer(dbar, dbar)
        terms = counts[idx] / counts[idx].sum(axis=1, keepdims=True)
        out["means"][j] = means[ctr] + dbar
        out["within"][j], out["between"][j], out["covs"][j] = within, between, within + between
        out["scores"][j], out["counts"][j] = terms.mean(axis=0), counts[idx].mean(axis=0)
        t = np.abs(covs[idx]).mean(axis=0) + np.abs(dd).mean(axis=0) + np.abs(np.outer(dbar, dbar))
        for key in ("covs", "within", "between"):
            bound[key][j] = EPS * t
        bound["means"][j] = EPS * (np.abs(means[ctr]) + np.abs(d).mean(axis=0))
        bound["scores"][j] = EPS * np.abs(terms).mean(axis=0)
        bound["counts"][j] = EPS * np.abs(counts[idx]).mean(axis=0)
    out["bound"] = bound
    return out


def uncentred_mixture(means, covs, idx):
    """The textbook moment form of the same mixture, (1/n) sum (Sigma_i + mu_i mu_i^T) - mu mu^T, in float64: (mean, cov)."""
    mu = np.asarray(means, np.float64)[idx]
    sg = np.asarray(covs, np.float64)[idx]
    mean = mu.mean(axis=0)
    return mean, (sg + mu[:, :, None] * mu[:, None, :]).mean(axis=0) - np.outer(mean, mean)


def centre_scores_f32(counts_row):
    """counts_c / sum_j counts_cj in float32, the sum taken for j ascending: the quotient the centre method is within 2^-23 of."""
    row = np.asarray(counts_row, np.float32)
    s = np.float32(0.0)
    for v in row:
        s = np.float32(s + v)
    return row / s
