"""Host: the float64 statement of 'regression_nll' and 'regression_energy' (bayes_od_rc_amd/proper_losses.py)
-- the twin the device kernels are compared with (test_gpu_proper_losses.py) -- against an independent torch statement
(tests/proper_loss_reference.py), against the scoring rules `offline_eval scores` reports, and against the energy score's
closed form; and the two new names through the loss tables."""
import math

import numpy as np
import pytest

from bayes_od_rc_amd import proper_losses as pl, scoring_rules as sr
from bayes_od_rc_amd.prob_detection_quality import _VUHW_TO_CORNERS

import proper_loss_reference as ref

SEED = 0x0123456789ABCDEF
BOX, BOX_T, ANCHORS, COV = ref.raw_rows()
N = BOX.shape[0]
IMAGE_IDS = 7 + np.arange(N) // 9
ANCHOR_IDS = (np.arange(N) * 7919) % 50000


def _twin(kind, m):
    """The twin on the shared rows, its gradient chained through the decode: (s_cmp, s_reg, d/dbox, d/dcov)."""
    pb, dpb = pl.decode_rows_np(BOX, ANCHORS)
    tb, _ = pl.decode_rows_np(BOX_T, ANCHORS)
    s_cmp, s_reg, d_pb, d_c = pl.proper_loss_rows_np(pb, tb, COV, IMAGE_IDS, ANCHOR_IDS, kind, m, SEED)
    return s_cmp, s_reg, d_pb * dpb, d_c


@pytest.mark.parametrize("kind,m", [(4, 64), (5, 2), (5, 64), (5, 65)])
def test_twin_and_its_gradient_equal_autograd(kind, m):
    """Both sides float64: 1e-9 (|want| + 1), the bound test_gpu_scores.py uses for the same kind of comparison."""
    normals = pl.loss_normals(IMAGE_IDS, ANCHOR_IDS, m, SEED) if kind == 5 else None
    want = ref.autograd_rows(kind, BOX, BOX_T, ANCHORS, COV, normals)
    got = _twin(kind, m)
    for name, g, w in zip(("s_cmp", "s_reg", "d_box", "d_cov"), got, want):
        assert g.shape == w.shape and np.isfinite(g).all(), name
        dev = np.abs(g - w) / (np.abs(w) + 1.0)
        print("kind %d M=%d %s: largest deviation %.2e" % (kind, m, name, dev.max()))
        assert (dev <= 1e-9).all(), (name, np.argwhere(dev > 1e-9)[:5], float(dev.max()))
    e = ref.N_RANDOM
    d_box = got[2]
    assert (d_box[e + 4, 2:] == 0.0).all() and (d_box[e + 5, 2:] == 0.0).all()      # a clipped coordinate passes no gradient
    assert (d_box[e + 4, :2] != 0.0).all() and (d_box[e + 6] != 0.0).all()          # (a clipped target clips nothing of p)
    if kind == 5:
        assert (got[1] == 0.0).all()


def test_nll_is_the_nll_scores_reports():
    """|det T| = 1: s_cmp + s_reg + 2 ln 2pi is column 0 of score_rows_np on (T pb, T Sigma T^T, T tb)."""
    T = _VUHW_TO_CORNERS
    pb, _ = pl.decode_rows_np(BOX, ANCHORS)
    tb, _ = pl.decode_rows_np(BOX_T, ANCHORS)
    s_cmp, s_reg, _, _ = pl.proper_loss_rows_np(pb, tb, COV, IMAGE_IDS, ANCHOR_IDS, 4)
    out, status = sr.score_rows_np(pb @ T.T, T @ pl.covariance_np(COV) @ T.T, tb @ T.T, np.arange(N), num_samples=2, seed=0)
    assert not status.any()
    got, want = s_cmp + s_reg + 2.0 * math.log(2.0 * math.pi), out[:, 0]
    dev = np.abs(got - want) / (np.abs(want) + 1.0)
    print("largest deviation %.2e" % dev.max())
    assert (dev <= 1e-9).all(), (np.argwhere(dev > 1e-9)[:5], float(dev.max()))


def test_energy_score_of_an_isotropic_row_has_its_closed_form():
    """Sigma = sigma^2 I and pb = tb: E = sigma (E|n4| - 0.5 E|n4 - n4'|), E|n4| = 3 sqrt(2 pi) / 4 and the difference of two
    independent 4-vectors is sqrt(2) times a standard one.  |T x| = |x| fails for T (it is no rotation), so the row lives in
    a basis where it does: the check is on the estimator's two coefficients, and T's columns are orthogonal with squared
    lengths (2, 2, 1/2, 1/2) -- sigma_k = sigma / |T e_k| makes T y isotropic with scale sigma."""
    sigma, rows, m = 3.0, 200, 1024
    col = np.sqrt(np.sum(_VUHW_TO_CORNERS ** 2, axis=0))
    cov = np.zeros((rows, 10))
    cov[:, [4, 9, 5, 0]] = 2.0 * np.log(sigma / col)
    pb = np.tile([300.0, 400.0, 80.0, 60.0], (rows, 1))
    s_cmp, s_reg, _, _ = pl.proper_loss_rows_np(pb, pb, cov, np.full(rows, 5), np.arange(rows), 5, m, SEED)
    want = sigma * (3.0 * math.sqrt(2.0 * math.pi) / 4.0) * (1.0 - math.sqrt(2.0) / 2.0)
    mean, sem = s_cmp.mean(), s_cmp.std(ddof=1) / math.sqrt(rows)
    print("mean %.6f want %.6f standard error %.6f" % (mean, want, sem))
    assert abs(mean - want) <= 4.0 * sem
    assert (s_reg == 0.0).all()


def test_new_names_through_the_loss_tables():
    from bayes_od_rc_amd import run_training
    from bayes_od_rc_amd.model import RetinaNetModel, loss_from_sums
    cfg = {"output_names": ["classification", "regression", "regression_covar"], "mc_dropout_samples": 10,
           "header": {"dropout_rate": 0.3, "num_classes": 7, "anchors_per_location": 9, "l2_norm_rate": "1e-3"},
           "losses": {"loss_names": ["classification", "regression_nll"], "loss_weights": [5.0, 1.0]}}
    assert RetinaNetModel(cfg).loss_kinds() == (True, 4)
    cfg["losses"]["loss_names"] = ["regression_energy"]
    assert RetinaNetModel(cfg).loss_kinds() == (False, 5)
    cfg["losses"]["loss_names"] = ["classification", "regression_nll", "regression_energy"]
    with pytest.raises(ValueError):
        RetinaNetModel(cfg).loss_kinds()
    cfg["losses"]["loss_names"] = ["classification", "regression_covar", "regression_energy"]
    with pytest.raises(ValueError):
        RetinaNetModel(cfg).loss_kinds()
    assert run_training._REG_KIND["regression_nll"] == 4 and run_training._REG_KIND["regression_energy"] == 5
    assert RetinaNetModel._REG_KIND == run_training._REG_KIND
    sums = [12.0, 6.0, 3.0, 4.0]
    total, d = loss_from_sums(["classification", "regression_nll"], [5.0, 2.0], sums)
    assert d == {"cls_loss": 15.0, "reg_loss": 1.5, "covariance_loss": 0.75} and total == 15.0 + 2.0 * 2.25
    total, d = loss_from_sums(["classification", "regression_energy"], [5.0, 2.0], [12.0, 6.0, 0.0, 4.0])
    assert d == {"cls_loss": 15.0, "reg_loss": 1.5, "covariance_loss": 0.0} and total == 15.0 + 3.0
