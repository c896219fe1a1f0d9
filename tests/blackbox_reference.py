"""Black-box MC dropout (include/bayesod.h, bod_set_uncertainty_method) restated in NumPy float64: the aleatoric
matrix of one sample's covariance parameters, and stage 2 -- the greedy pool merge -- with the bound a float32 kernel is held to
for every output entry, plus the pools the tests feed both sides.  Nothing here calls the code under test.

Stage 2, per image, on the pool of sample detections (pooled index n * Kmax + rank): the unassigned detection with the highest top
score is a centre c (ties: the lower pooled index); members = c and every unassigned i with iou_plus1(corners_c, corners_i) > theta;
with n members and d_i = mu_i - mu_c:  dbar = (1/n) sum d_i, mean = mu_c + dbar, within = (1/n) sum cov_i,
between = (sum d_i d_i^T - n dbar dbar^T) / (n - 1) (exactly 0 for n = 1), cov = within + between, counts = sum score_i,
scores = counts / n; a cluster below min_members emits nothing and keeps its members; at most Kmax clusters are emitted.

Roundings on bb_merge_kernel's longest path to an entry of `between`, the deepest one:
  1   d_i = mu_i - mu_c
  1   the product d_r d_q
  s   the thread's serial chain: it owns every 256th pool entry, so s <= min(n, ceil(P / 256)) adds
  6   wave butterfly
  2   (w0 + w1) + (w2 + w3)
  6   dbar = sum / n (1), dbar_r dbar_q (1), n * that (1), the subtraction (1), / (n - 1) (1), cov = within + between (1)
so ROUNDINGS(n, P) = min(n, ceil(P / 256)) + 16, and the bound of an entry is ROUNDINGS * 2^-24 * (the sum of the absolute values
of the entry's terms, absolute values taken inside the mean too) * 4, the factor tests/merge_reference.py uses.  `members`, the
centres and the emission order are exact.

The aleatoric matrix L D L^T, L = inv(unit_lower(params)), D = exp(diag): expf is within 2 ulp (2 roundings), an entry of L goes
through at most 5 roundings (l32 * (l21 * l10 + l20) + l31 * l10 + l30), an entry of the product through two of those, two
multiplications and three adds, and the KITTI rescale adds two: ALEATORIC_ROUNDINGS = 2 + 5 + 5 + 2 + 3 + 2 = 19, times 2^-24, times
the sum of |L_ik| D_k |L_jk| with the absolute values taken inside L as well, times 4.
"""
import numpy as np

import post_reference

ALEATORIC_ROUNDINGS = 19
AFFINITY_GUARD = 1e-3
SCORE_GAP = 1e-6


def roundings(n, pool):
    return min(int(n), -(-int(pool) // 256)) + 16


def aleatoric_matrix(params, use_full_covar=True, has_covar_head=True, scale=None):
    """params [m,10] (the head's raw output, pre fill_triangular) -> (Sigma [m,4,4] float64, bound [m,4,4]).  scale: the KITTI
    factors (sh, sw) or None."""
    x = np.asarray(params, np.float64).reshape(-1, 10)
    m = x.shape[0]
    if not has_covar_head:
        return np.zeros((m, 4, 4)), np.zeros((m, 4, 4))
    d = np.exp(np.stack([x[:, 4], x[:, 9], x[:, 5], x[:, 0]], axis=1))
    lower = np.zeros((m, 4, 4))
    for i in range(4):
        lower[:, i, i] = 1.0
    if use_full_covar:
        lower[:, 1, 0], lower[:, 2, 0], lower[:, 2, 1] = x[:, 8], x[:, 7], x[:, 6]
        lower[:, 3, 0], lower[:, 3, 1], lower[:, 3, 2] = x[:, 3], x[:, 2], x[:, 1]
    li = np.linalg.inv(lower)
    # |inv| with the absolute values taken inside: the inverse of the unit-lower matrix with -|l| below the diagonal is the sum of
    # the absolute values of every path product
    ali = np.linalg.inv(2.0 * np.eye(4) - np.abs(lower))
    sigma = np.einsum("mik,mk,mjk->mij", li, d, li)
    mag = np.einsum("mik,mk,mjk->mij", ali, d, ali)
    if scale is not None:
        sc = np.array([scale[0], scale[1], scale[0], scale[1]], np.float64)
        sigma = sigma * sc[:, None] * sc[None, :]
        mag = mag * np.abs(sc[:, None] * sc[None, :])
    return sigma, ALEATORIC_ROUNDINGS * 2.0 ** -24 * 4.0 * mag


def corners_f32(means):
    """vuhw_to_vuvu in float32, as the device forms the pool's corners from the float32 means."""
    m = np.asarray(means, np.float32).reshape(-1, 4)
    two = np.float32(2.0)
    return np.stack([m[:, 0] - m[:, 2] / two, m[:, 1] - m[:, 3] / two, m[:, 0] + m[:, 2] / two, m[:, 1] + m[:, 3] / two], axis=1)


def pool_arrays(samples, kmax):
    """samples: list over n of dicts {'scores' [k,C], 'means' [k,4], 'covs' [k,4,4]} -> pooled index [m], scores, means, covs."""
    idx, sc, mu, cv = [], [], [], []
    for n, s in enumerate(samples):
        k = len(s["scores"])
        assert k <= kmax
        idx.append(n * kmax + np.arange(k))
        sc.append(np.asarray(s["scores"], np.float32).reshape(k, np.shape(s["scores"])[-1]))
        mu.append(np.asarray(s["means"], np.float32).reshape(k, 4))
        cv.append(np.asarray(s["covs"], np.float32).reshape(k, 4, 4))
    return np.concatenate(idx), np.concatenate(sc), np.concatenate(mu), np.concatenate(cv)


def check_pool_conditions(samples, kmax, thr):
    """The two conditions every generated pool satisfies by construction: every pairwise affinity at least AFFINITY_GUARD away from
    the threshold, all top scores at least SCORE_GAP apart."""
    _, sc, mu, _ = pool_arrays(samples, kmax)
    if len(sc) < 2:
        return
    aff = post_reference.iou_plus1(corners_f32(mu))
    off = ~np.eye(len(sc), dtype=bool)
    assert np.abs(aff[off] - thr).min() >= AFFINITY_GUARD, np.abs(aff[off] - thr).min()
    top = np.sort(sc.max(axis=1).astype(np.float64))
    assert np.diff(top).min() >= SCORE_GAP, np.diff(top).min()


def pool_merge_reference(samples, kmax, thr=0.5, min_members=1):
    """float64 on the float32-valued inputs.  Returns scores [k,C], means [k,4], covs / within / between [k,4,4], counts [k,C],
    members [k], centre [k] (pooled indices) in emission order, and `bound`: key -> the absolute error allowed, entry by entry."""
    pidx, sc32, mu32, cv32 = pool_arrays(samples, kmax)
    pool = len(samples) * kmax
    c = sc32.shape[1]
    sc, mu, cv = sc32.astype(np.float64), mu32.astype(np.float64), cv32.astype(np.float64)
    aff = post_reference.iou_plus1(corners_f32(mu32)) if len(sc) else np.zeros((0, 0))
    top = sc32.max(axis=1) if len(sc) else np.zeros(0, np.float32)
    free = np.ones(len(sc), bool)
    keys = ("scores", "means", "covs", "counts", "within", "between")
    rows = {k: [] for k in keys + ("members", "centre")}
    bnd = {k: [] for k in keys}
    while free.any() and len(rows["members"]) < kmax:
        cand = np.nonzero(free)[0]
        best = top[cand].max()
        ctr = cand[top[cand] == best][np.argmin(pidx[cand[top[cand] == best]])]
        member = free & (aff[ctr] > thr)
        member[ctr] = True
        free &= ~member
        idx = np.nonzero(member)[0]
        n = len(idx)
        if n < min_members:
            continue
        eps = roundings(n, pool) * 2.0 ** -24 * 4.0
        d = mu[idx] - mu[ctr]
        dbar = d.mean(axis=0)
        abar = np.abs(d).mean(axis=0)
        dd = d[:, :, None] * d[:, None, :]
        within = cv[idx].mean(axis=0)
        if n >= 2:
            between = (dd.sum(axis=0) - n * np.outer(dbar, dbar)) / (n - 1)
            tb = (np.abs(dd).sum(axis=0) + n * np.outer(abar, abar)) / (n - 1)
        else:
            between, tb = np.zeros((4, 4)), np.zeros((4, 4))
        tw = np.abs(cv[idx]).mean(axis=0)
        rows["means"].append(mu[ctr] + dbar)
        bnd["means"].append(eps * (np.abs(mu[ctr]) + abar))
        rows["within"].append(within); bnd["within"].append(eps * tw)
        rows["between"].append(between); bnd["between"].append(eps * tb)
        rows["covs"].append(within + between); bnd["covs"].append(eps * (tw + tb))
        rows["counts"].append(sc[idx].sum(axis=0)); bnd["counts"].append(eps * np.abs(sc[idx]).sum(axis=0))
        rows["scores"].append(sc[idx].sum(axis=0) / n); bnd["scores"].append(eps * np.abs(sc[idx]).sum(axis=0) / n)
        rows["members"].append(n)
        rows["centre"].append(int(pidx[ctr]))
    shapes = {"scores": (0, c), "means": (0, 4), "covs": (0, 4, 4), "counts": (0, c), "within": (0, 4, 4), "between": (0, 4, 4)}
    out = {k: (np.stack(rows[k]) if rows[k] else np.zeros(shapes[k])) for k in keys}
    out["members"] = np.asarray(rows["members"], np.int32)
    out["centre"] = np.asarray(rows["centre"], np.int32)
    out["bound"] = {k: (np.stack(bnd[k]) if bnd[k] else np.zeros(shapes[k])) for k in keys}
    return out


def clustered_pool(rng, clusters, c, n_samples, kmax, thr=0.5):
    """A pool of sample detections in clusters.  `clusters`: a list of lists of sample indices, one entry per member (so [0, 1, 2] is
    a cluster with one member from each of three samples, [1, 1] two members from the same sample, [2] a detection alone).  Cluster
    k lives in cell k of a wide canvas: its members are its first box jittered by a pixel (IoU ~ 0.9), so every pair inside a cell
    is far above the threshold and every pair across cells is at 0; the top scores are distinct points of a grid with spacing
    >= 2e-5.  Both conditions are asserted.  Detections are dealt to their samples in shuffled order (the rank within a sample carries
    no meaning for stage 2).  Returns the list over samples of {'scores', 'means', 'covs', 'anchor_index'}, float32."""
    m = sum(len(cl) for cl in clusters)
    tops = 0.55 + 0.4 * (rng.permutation(m) + rng.uniform(0.0, 0.5, m)) / m
    per = [[] for _ in range(n_samples)]
    t = 0
    for k, cl in enumerate(clusters):
        base = np.array([80.0 + 150.0 * (k // 40), 80.0 + 150.0 * (k % 40), rng.uniform(30, 60), rng.uniform(30, 60)])
        for j, n in enumerate(cl):
            box = base if j == 0 else np.concatenate([base[:2] + rng.normal(0, 1.0, 2), base[2:] * np.exp(rng.normal(0, 0.02, 2))])
            a = rng.normal(size=(4, 4))
            cov = a @ a.T + 2.0 * np.eye(4)
            row = (1.0 - tops[t]) * rng.dirichlet(np.ones(c - 1))
            row = np.insert(row, rng.integers(0, c - 1), tops[t])          # the top score at a foreground class
            per[n].append((row, box, cov, rng.integers(0, 3069)))
            t += 1
    out = []
    for n in range(n_samples):
        order = rng.permutation(len(per[n]))
        assert len(order) <= kmax, (n, len(order))
        rows = [per[n][i] for i in order]
        covs = np.array([r[2] for r in rows], np.float32).reshape(-1, 4, 4)
        covs = np.tril(covs) + np.tril(covs, -1).transpose(0, 2, 1)
        out.append({"scores": np.array([r[0] for r in rows], np.float32).reshape(-1, c),
                    "means": np.array([r[1] for r in rows], np.float32).reshape(-1, 4), "covs": covs,
                    "anchor_index": np.array([r[3] for r in rows], np.int32).reshape(-1)})
    check_pool_conditions(out, kmax, thr)
    return out
