"""Host statement of the two proper-scoring-rule training losses (device: csrc/loss_kernels.hip).

Per positive anchor, with ``pb`` / ``tb`` the decoded prediction and target in vuhw pixels, ``e = pb - tb``, ``c[0..9]`` the
raw covariance parameters, ``ld = (c4, c9, c5, c0)``, ``A1`` the unit-lower matrix with rows (1), (c8, 1), (c7, c6, 1),
(c3, c2, c1, 1) and ``Sigma = A1^-1 diag(exp ld) A1^-T`` (the covariance inference_utils builds from the same numbers):

* kind 4 'regression_nll':    ``s_cmp = 0.5 sum_k exp(-ld_k) r_k^2`` with ``r = A1 e``;  ``s_reg = 0.5 sum_k ld_k``
  (``s_cmp + s_reg + 2 ln 2pi`` is the Gaussian negative log-likelihood of ``tb``).
* kind 5 'regression_energy': ``A1 y_i = exp(ld/2) o n_i``, ``z_i = T (pb + y_i)``, ``g = T tb`` (T: vuhw -> corners),
  ``s_cmp = (1/M) sum_{i<M} |z_i - g| - 1/(2(M-1)) sum_{i<M-1} |z_i - z_{i+1}|``;  ``s_reg = 0``.

The normals extend the Philox contract of scoring_rules.py with a tag of their own: sample i of (image id, anchor a) is one
call ``philox4x32_10(i, a, LOSS_TAG, image id, seed_lo, seed_hi)``, turned into four normals as there.  NumPy, float64.
"""
import math

import numpy as np

from .prob_detection_quality import _VUHW_TO_CORNERS
from .scoring_rules import philox4x32_10

LOSS_TAG = 0x0010555E
MIN_SAMPLES, MAX_SAMPLES, DEFAULT_SAMPLES = 2, 1024, 64
REG_KIND_NLL, REG_KIND_ENERGY = 4, 5

_DIAG = (4, 9, 5, 0)                                           # ld_k = c[_DIAG[k]]
_OFF = ((1, 0, 8), (2, 0, 7), (2, 1, 6), (3, 0, 3), (3, 1, 2), (3, 2, 1))      # A1[k][j] = c[index]


def loss_normals(image_ids, anchor_ids, num_samples, seed):
    """The contract's standard normals [rows, num_samples, 4] (float64) of the rows (image id, anchor)."""
    img = np.asarray(image_ids, dtype=np.uint64).reshape(-1, 1)
    an = np.asarray(anchor_ids, dtype=np.uint64).reshape(-1, 1)
    i = np.arange(int(num_samples), dtype=np.uint64)[None, :]
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    x, y, z, w = philox4x32_10(i, an, np.uint64(LOSS_TAG), img, seed & 0xFFFFFFFF, seed >> 32)
    u = [(t.astype(np.float64) + 0.5) * 2.0 ** -32 for t in (x, y, z, w)]
    r0, r1 = np.sqrt(-2.0 * np.log(u[0])), np.sqrt(-2.0 * np.log(u[2]))
    a0, a1 = (2.0 * math.pi) * u[1], (2.0 * math.pi) * u[3]
    return np.stack([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1), r1 * np.sin(a1)], axis=-1)


def decode_rows_np(box, anchors):
    """The decode of the covariance losses (retinanet_model.py:262-285): box-head values [n,4] and their anchors [n,4]
    (v, u, h, w) -> (decoded vuhw [n,4], d decoded / d box [n,4]); a coordinate whose exp leaves [1e-4, 1e4] is clipped
    and passes no gradient."""
    box, anchors = np.asarray(box, np.float64).reshape(-1, 4), np.asarray(anchors, np.float64).reshape(-1, 4)
    out, grad = np.empty_like(box), np.empty_like(box)
    with np.errstate(over='ignore'):
        for k in (0, 1):
            out[:, k] = anchors[:, 2 + k] * box[:, k] / 10.0 + anchors[:, k]
            grad[:, k] = anchors[:, 2 + k] / 10.0
            ex = np.exp(box[:, 2 + k] / 5.0)
            out[:, 2 + k] = anchors[:, 2 + k] * np.clip(ex, 1e-4, 1e4)
            grad[:, 2 + k] = np.where((ex >= 1e-4) & (ex <= 1e4), anchors[:, 2 + k] * np.where(np.isfinite(ex), ex, 0.0) / 5.0, 0.0)
    return out, grad


def unit_lower(cov_params):
    """A1 [n,4,4] of the raw parameters [n,10]."""
    c = np.asarray(cov_params, np.float64).reshape(-1, 10)
    a1 = np.tile(np.eye(4), (c.shape[0], 1, 1))
    for k, j, q in _OFF:
        a1[:, k, j] = c[:, q]
    return a1


def covariance_np(cov_params):
    """Sigma = A1^-1 diag(exp ld) A1^-T [n,4,4]."""
    c = np.asarray(cov_params, np.float64).reshape(-1, 10)
    inv = np.linalg.inv(unit_lower(c))
    return np.einsum('nij,nj,nkj->nik', inv, np.exp(c[:, list(_DIAG)]), inv)


def _unit(x):
    """x / |x| along the last axis, 0 where |x| = 0."""
    n = np.sqrt(np.sum(x * x, axis=-1, keepdims=True))
    return np.divide(x, n, out=np.zeros_like(x), where=n > 0)


def proper_loss_abs_terms_np(pb, tb, cov_params, image_ids, anchor_ids, kind, num_samples=DEFAULT_SAMPLES, seed=0):
    """Per row the sum of the ABSOLUTE terms ``s_cmp`` and ``s_reg`` are made of -- the scale a float32 evaluation's error is
    measured in: kind 4 ``(s_cmp, 0.5 sum |ld_k|)``, kind 5 ``((1/M) sum |z_i - g| + 1/(2(M-1)) sum |z_i - z_{i+1}|, 0)``."""
    c = np.asarray(cov_params, np.float64).reshape(-1, 10)
    s_cmp = proper_loss_rows_np(pb, tb, c, image_ids, anchor_ids, kind, num_samples, seed)[0]
    if kind == REG_KIND_NLL:
        return s_cmp, 0.5 * np.sum(np.abs(c[:, list(_DIAG)]), axis=1)
    # s_cmp = a - b with both parts >= 0; a = (1/M) sum |z_i - g| follows from the same rows with the neighbour part removed
    e = np.asarray(pb, np.float64).reshape(-1, 4) - np.asarray(tb, np.float64).reshape(-1, 4)
    s = np.exp(0.5 * c[:, list(_DIAG)])[:, None, :] * loss_normals(image_ids, anchor_ids, int(num_samples), seed)
    a1 = unit_lower(c)
    y = np.zeros_like(s)
    for k in range(4):
        y[:, :, k] = s[:, :, k] - np.einsum('nj,nij->ni', a1[:, k, :k], y[:, :, :k])
    za = (e[:, None, :] + y) @ _VUHW_TO_CORNERS.T
    a = np.sqrt(np.sum(za * za, -1)).sum(1) / int(num_samples)
    return 2.0 * a - s_cmp, np.zeros(c.shape[0])


def proper_loss_rows_np(pb, tb, cov_params, image_ids, anchor_ids, kind, num_samples=DEFAULT_SAMPLES, seed=0):
    """Per row ``(s_cmp [n], s_reg [n], d/dpb [n,4], d/dcov_params [n,10])`` of ``s_cmp + s_reg`` in float64, from the
    formulas of the module's docstring.  ``pb`` / ``tb`` [n,4] are decoded vuhw boxes (the gradient through the decode is
    ``decode_rows_np``'s second value); kind 4 ignores ids, sample count and seed."""
    pb, tb = np.asarray(pb, np.float64).reshape(-1, 4), np.asarray(tb, np.float64).reshape(-1, 4)
    c = np.asarray(cov_params, np.float64).reshape(-1, 10)
    n = pb.shape[0]
    if tb.shape[0] != n or c.shape[0] != n:
        raise ValueError("pb, tb and cov_params must have one row per anchor")
    e = pb - tb
    ld = c[:, list(_DIAG)]
    a1 = unit_lower(c)
    d_pb, d_c = np.zeros((n, 4)), np.zeros((n, 10))
    if kind == REG_KIND_NLL:
        r = np.einsum('nkj,nj->nk', a1, e)
        u = np.exp(-ld) * r
        s_cmp, s_reg = 0.5 * np.sum(u * r, axis=1), 0.5 * np.sum(ld, axis=1)
        d_pb = np.einsum('nkj,nk->nj', a1, u)
        d_c[:, list(_DIAG)] = -0.5 * u * r + 0.5
        for k, j, q in _OFF:
            d_c[:, q] = u[:, k] * e[:, j]
        return s_cmp, s_reg, d_pb, d_c
    if kind != REG_KIND_ENERGY:
        raise ValueError("kind must be 4 (regression_nll) or 5 (regression_energy), got %r" % (kind,))
    m = int(num_samples)
    if not MIN_SAMPLES <= m <= MAX_SAMPLES:
        raise ValueError("num_samples %d outside [%d, %d]" % (m, MIN_SAMPLES, MAX_SAMPLES))
    if n == 0:
        return np.zeros(0), np.zeros(0), d_pb, d_c
    T = _VUHW_TO_CORNERS
    s = np.exp(0.5 * ld)[:, None, :] * loss_normals(image_ids, anchor_ids, m, seed)                  # [n,M,4]
    y = np.zeros_like(s)
    for k in range(4):                                              # forward substitution A1 y = s
        y[:, :, k] = s[:, :, k] - np.einsum('nj,nij->ni', a1[:, k, :k], y[:, :, :k])
    za = (e[:, None, :] + y) @ T.T                                  # z_i - g
    zb = (y[:, 1:] - y[:, :-1]) @ T.T                               # z_{i+1} - z_i
    s_cmp = np.sqrt(np.sum(za * za, -1)).sum(1) / m - np.sqrt(np.sum(zb * zb, -1)).sum(1) / (2.0 * (m - 1))
    w = _unit(za) / m
    ub = _unit(zb) / (2.0 * (m - 1))
    w[:, 1:] -= ub                                                  # u(z_i - z_{i-1})
    w[:, :-1] += ub                                                 # u(z_i - z_{i+1}) = -u(z_{i+1} - z_i)
    v = w @ T                                                       # T^T w_i
    q = np.zeros_like(v)
    for k in range(3, -1, -1):                                      # back substitution A1^T q = v
        q[:, :, k] = v[:, :, k] - np.einsum('nj,nij->ni', a1[:, k + 1:, k], q[:, :, k + 1:])
    d_pb = v.sum(1)
    d_c[:, list(_DIAG)] = 0.5 * np.sum(q * s, axis=1)
    for k, j, qi in _OFF:
        d_c[:, qi] = -np.sum(q[:, :, k] * y[:, :, j], axis=1)
    return s_cmp, np.zeros(n), d_pb, d_c
