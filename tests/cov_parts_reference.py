"""TEST INFRASTRUCTURE shared by tests/test_cov_parts_host.py and tests/test_gpu_cov_parts.py: the float64 statement of the
covariance parts (include/bayesod.h) -- the three terms every posterior covariance and every fused detection
covariance is the sum of.  Nothing here calls the code under test.

Both fusion steps are linear in the means they fuse, so the covariance of the fused mean splits exactly by where the noise of
those means came from: the epistemic term E (sample covariance over the MC samples), the aleatoric term A (covariance head) and
the Gaussian prior."""
import numpy as np

PART_NAMES = ("epistemic", "aleatoric", "prior")


def _t(m):
    return np.transpose(m, (0, 2, 1))


def posterior_parts(debug, bayes_od_config, scale=None):
    """Parts [M,3,4,4] (float64) of the posterior covariances of ``oracle.bayes_od.bayes_od_posterior(..., return_debug=True)``.

    With lik = (10 A + E) / 11 = a + e and the prior iso_var * I:  P = (lik^-1 + I / iso_var)^-1, the gain of the posterior mean
    on the likelihood's mean is G = P lik^-1 = I - P / iso_var, and  P = G e G^T + G a G^T + P P / iso_var.  Without a Gaussian
    prior G = I and the prior term is 0.  ``scale`` = (sh, sw): KITTI's S = diag(sh, sw, sh, sw), every term becomes S X S^T."""
    e = np.asarray(debug["cov_epi"], np.float64) / 11.0
    a = 10.0 * np.asarray(debug["cov_al"], np.float64) / 11.0
    m = e.shape[0]
    eye = np.eye(4)[None]
    if bayes_od_config["gaussian_prior"]["type"] == "isotropic" and m:
        iso = float(bayes_od_config["gaussian_prior"]["isotropic_variance"])
        p = np.linalg.inv(np.linalg.inv(np.asarray(debug["cov_lik"], np.float64)) + eye / iso)
        g = eye - p / iso
        pri = p @ p / iso
    else:
        g = np.tile(eye, (m, 1, 1))
        pri = np.zeros_like(e)
    parts = np.stack([g @ e @ _t(g), g @ a @ _t(g), pri], axis=1)
    if scale is not None:
        s = np.diag(np.tile(np.asarray(scale, np.float64), 2))
        parts = s[None, None] @ parts @ s.T[None, None]
    return parts


def kitti_scale(orig_size, net_size):
    """(sh, sw) as oracle.bayes_od rounds them: orig / net in float64, stored as float32."""
    s = np.asarray(orig_size[:2], np.float64) / np.asarray(net_size[:2], np.float64)
    return s.astype(np.float32).astype(np.float64)


def cluster_parts(covs, parts, centres, affinity, affinity_threshold=0.7):
    """Parts [K,3,4,4] (float64) of ``oracle.clustering.bayes_od_clustering``'s output covariances.  Members of centre k are
    ``affinity[:, centre] > affinity_threshold`` (the oracle's rule, inference_utils.py:316); with P_i = covs_i^-1 and
    F = (sum P_i)^-1 the fused mean is F sum P_i mu_i, so each part is  70 F (sum P_i X_i P_i) F  and the three sum to 70 F."""
    from oracle.clustering import COV_CALIBRATION
    covs = np.asarray(covs, np.float64)
    parts = np.asarray(parts, np.float64)
    out = []
    for centre in centres:
        members = np.asarray(affinity)[:, centre] > affinity_threshold
        precs = np.linalg.inv(covs[members])
        f = np.linalg.inv(precs.sum(axis=0))
        s = np.einsum("mij,mpjk,mkl->pil", precs, parts[members], precs)
        out.append(COV_CALIBRATION * (f[None] @ s @ f[None]))
    return np.asarray(out).reshape(-1, 3, 4, 4)


def parts_error(got, ref, total):
    """The project's metric for posterior covariances (tests/test_gpu_post.py REL_TOL) per entry of the parts [M,3,4,4]:
    |got - ref| / (|ref| + floor), floor = 1 % of the largest entry of the row's TOTAL covariance [M,4,4] -- a part that is
    nearly zero is judged on the scale of the matrix it belongs to.  Returns the maximum (0 for no rows)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if got.size == 0:
        return 0.0
    floor = np.abs(np.asarray(total, np.float64)).reshape(len(ref), -1).max(axis=1)[:, None, None, None] * 1e-2
    return float((np.abs(got - ref) / (np.abs(ref) + floor)).max())
