"""GPU parity of the Bayesian post-processing stages, each fed IDENTICAL inputs through the C ABI
(bod_set_raw / bod_set_posterior / bod_set_nms) and compared with the oracle:

  posterior   inference_utils.py:25-202   vs oracle.bayes_od.bayes_od_posterior
  soft-NMS    inference_utils.py:204-212  vs oracle.nms.soft_nms (bit-exact index lists)
  clustering  inference_utils.py:285-364  vs the reference's own outputs (tests/golden/clustering.npz) and oracle.clustering

The second half of the file takes each stage to its configuration corners and size edges (4 classes, every prior pair, no
covariance head, empty / full kept sets, the statistics route, the storage switches of the NMS, cluster sizes around the block
stride, exact KL ties); its shared inputs come from tests/post_reference.py.
"""
import numpy as np
import pytest

import post_reference
from conftest import ANCHOR_CFG, BAYES_CFG, NMS_CFG, compare_posterior, rel_err

pytestmark = pytest.mark.gpu
REL_TOL = 1e-3          # BASELINE.json north_star


def _engine(hw=(128, 128), batch=1, n=5, weights=True, **kw):
    from bayes_od_rc_amd import synthetic
    from bayes_od_rc_amd.engine import Engine, make_config
    from bayes_od_rc_amd.anchor_generator import FpnAnchorGenerator
    eng = Engine(make_config(hw, batch=batch, mc_samples=n, **kw))
    if weights:                                   # (stage-level calls -- set_raw, set_posterior, set_statistics -- need none)
        eng.load_weights(synthetic.make_weights())
    anchors = FpnAnchorGenerator(ANCHOR_CFG).generate_all((hw[0], hw[1], 3))
    eng.set_anchors(anchors)
    return eng, anchors


_random_raw = post_reference.random_raw          # (c = 8, bg = +3: the stream these tests have always drawn)


@pytest.mark.parametrize("use_full_covar,ranking", [(True, "score"), (False, "score"), (True, "joint_entropy")])
def test_posterior_matches_oracle(use_full_covar, ranking):
    from oracle import bayes_od, philox, network
    bcfg = dict(BAYES_CFG, ranking_method=ranking)
    b, n = 2, 5
    eng, anchors = _engine(batch=b, n=n, use_full_covar=use_full_covar, bayes_od_config=bcfg)
    rng = np.random.default_rng(21)
    cls, box, cov = _random_raw(rng, b, n, eng.A)
    eng.set_raw(cls, box, cov)
    seed, first = 987654321987, 11
    eng.posterior(seed=seed, first_image_id=first)
    kept = eng.num_kept()
    for img in range(b):
        u = philox.categorical_uniforms(seed, first + img, eng.A)
        pred = {"anchors_class_predictions": cls[img], "anchors_box_predictions": box[img],
                "anchors_box_covar_predictions": network.fill_triangular_4(cov[img])}
        ref = bayes_od.bayes_od_posterior(pred, anchors, u, bcfg, use_full_covar=use_full_covar,
                                          dtype=np.float64, return_debug=True)
        got = eng.get_posterior(img)
        # anchors whose categorical draw sits within float32 rounding of a CDF boundary may
        # legitimately sample a neighbouring class: find them and exclude them from exactness
        cdf = np.cumsum(ref["mean_probs"], axis=1)
        t = u.astype(np.float64) * cdf[:, -1:]
        ambiguous = (np.abs(cdf[:, None, :] - t[:, :, None]).min(axis=(1, 2)) < 1e-5)
        ref_keep = ref["keep"]
        got_keep = np.zeros(eng.A, bool)
        got_keep[got["anchor_index"]] = True
        assert np.all(got["anchor_index"][1:] > got["anchor_index"][:-1])       # boolean_mask order
        diff = got_keep != ref_keep
        assert not np.any(diff & ~ambiguous), "filter mismatch on an unambiguous anchor"
        assert ambiguous.mean() < 5e-3
        assert kept[img] == got_keep.sum() and kept[img] > 20
        both = got_keep & ref_keep & ~ambiguous
        gi = np.searchsorted(got["anchor_index"], np.nonzero(both)[0])
        ri = np.cumsum(ref_keep)[both] - 1
        assert np.array_equal(got["counts"][gi], ref["counts"][ri].astype(np.float32))   # integers + 1/8: exact
        assert rel_err(got["score"][gi], ref["score"][ri], 1e-6) < REL_TOL
        mean_floor = 1.0                                  # pixels
        assert rel_err(got["means"][gi], ref["means"][ri][:, :, 0], mean_floor) < REL_TOL
        cov_ref = ref["covs"][ri]
        cov_floor = np.abs(cov_ref).reshape(len(ri), -1).max(axis=1)[:, None, None] * 1e-2
        err = np.abs(got["covs"][gi] - cov_ref) / (np.abs(cov_ref) + cov_floor)
        assert err.max() < REL_TOL, float(err.max())
        if ranking == "score":
            assert rel_err(got["ranking"][gi], ref["ranking"][ri], 1e-6) < REL_TOL
        elif not np.any(diff):
            # joint entropy = min-max-normalised information gains over the image's M boxes (inference_utils.py:171-200): the
            # Gaussian term is -0.5 log det(Sigma_post), taken through a double-precision Cholesky on the device, so the ranking
            # inherits only the covariances' own error (1e-3 of an entry -> <= 4e-3 of log det in the worst, aligned case; observed
            # far below) divided by the gains' range
            assert rel_err(got["ranking"], ref["ranking"], 1e-2) < REL_TOL
        # covariances are symmetric positive definite
        c = got["covs"]
        assert np.allclose(c, np.transpose(c, (0, 2, 1)), rtol=1e-5, atol=1e-7)
        assert np.all(np.linalg.eigvalsh(c.astype(np.float64)) > 0)


def test_posterior_kitti_rescale_and_no_priors():
    from oracle import bayes_od, philox, network
    bcfg = {"ranking_method": "score", "dirichlet_prior": {"type": "None"},
            "gaussian_prior": {"type": "None"}}
    n = 4
    eng, anchors = _engine(hw=(96, 160), batch=1, n=n, use_full_covar=True, bayes_od_config=bcfg,
                           dataset_name="kitti", orig_size=(375, 1242))
    rng = np.random.default_rng(4)
    cls, box, cov = _random_raw(rng, 1, n, eng.A)
    eng.set_raw(cls, box, cov)
    eng.posterior(seed=3, first_image_id=0)
    u = philox.categorical_uniforms(3, 0, eng.A)
    pred = {"anchors_class_predictions": cls[0], "anchors_box_predictions": box[0],
            "anchors_box_covar_predictions": network.fill_triangular_4(cov[0])}
    ref = bayes_od.bayes_od_posterior(pred, anchors, u, bcfg, use_full_covar=True, dataset_name="kitti",
                                      orig_size=(375, 1242, 3), net_size=(96, 160, 3), dtype=np.float64, return_debug=True)
    got = eng.get_posterior(0)
    # counts exact (no +1/C prior), means / covariances 1e-3 on every anchor off a CDF rounding boundary: never skipped
    checked, _ = compare_posterior(got, ref, u, tol=REL_TOL, min_checked=20)
    assert checked >= 20


def _posterior_like(rng, m, n_obj):
    centres = rng.uniform(40, 400, size=(n_obj, 2))
    dims = rng.uniform(20, 150, size=(n_obj, 2))
    which = rng.integers(0, n_obj, size=m)
    vu = centres[which] + rng.normal(scale=3.0, size=(m, 2))
    hw = dims[which] * np.exp(rng.normal(scale=0.06, size=(m, 2)))
    means = np.concatenate([vu, hw], 1).astype(np.float32)
    a = rng.normal(size=(m, 4, 4))
    covs = ((a @ np.transpose(a, (0, 2, 1)) + 0.5 * np.eye(4)) * 3.0).astype(np.float32)
    probs = rng.dirichlet(np.ones(8) * 0.6, size=m)
    counts = (np.stack([rng.multinomial(30, p) for p in probs]) + 0.125).astype(np.float32)
    score = counts / counts.sum(1, keepdims=True)
    return counts, means, covs, score.max(1).astype(np.float32)


@pytest.mark.parametrize("variant", ["A", "B"])
@pytest.mark.parametrize("m,n_obj", [(1, 1), (37, 3), (400, 25), (1500, 60), (5000, 200), (7000, 300)])
def test_soft_nms_bit_exact(variant, m, n_obj):
    """Index list identical to the restated NonMaxSuppressionV5 (oracle/nms.py)."""
    from oracle import nms, geometry
    eng, _ = _engine(hw=(256, 256), batch=2, n=2, nms_variant=variant)
    rng = np.random.default_rng(m)
    for img in range(2):
        counts, means, covs, ranking = _posterior_like(rng, m, n_obj)
        if img == 1:
            ranking[: m // 2] = ranking[0]            # exercise score ties (lowest index first)
        eng.set_posterior(img, counts, means, covs, ranking)
    eng.nms()
    rng = np.random.default_rng(m)
    for img in range(2):
        counts, means, covs, ranking = _posterior_like(rng, m, n_obj)
        if img == 1:
            ranking[: m // 2] = ranking[0]
        ref_idx, _ = nms.soft_nms(geometry.vuhw_to_vuvu(means), ranking, 100, 0.5, 0.5, variant=variant)
        got = eng.get_nms(img)
        assert np.array_equal(got, ref_idx), (img, got[:10], ref_idx[:10])


def test_nms_empty_image():
    eng, _ = _engine(batch=1, n=2)
    eng.set_posterior(0, np.zeros((0, 8)), np.zeros((0, 4)), np.zeros((0, 4, 4)), np.zeros((0,)))
    eng.nms()
    assert eng.get_nms(0).shape == (0,)
    eng.cluster_fuse()
    s, m, c, k = eng.get_detections(0)
    assert s.shape == (0, 8) and m.shape == (0, 4) and c.shape == (0, 4, 4) and k.shape == (0, 8)


def test_cluster_fuse_matches_reference_golden(golden_dir):
    """The reference's own bayes_od_clustering outputs (captured by import) are the expected values."""
    import os
    g = np.load(os.path.join(golden_dir, "clustering.npz"))
    eng8, _ = _engine(hw=(128, 128), batch=1, n=2, num_classes=8)
    eng4 = None
    for i in range(int(g["n_cases"])):
        t = "c%02d" % i
        counts, means, covs = g[t + "_counts"], g[t + "_means"], g[t + "_covs"]
        centres = g[t + "_centres"]
        if counts.shape[1] == 4:
            if eng4 is None:
                from bayes_od_rc_amd.engine import Engine, make_config
                eng4 = Engine(make_config((128, 128), batch=1, mc_samples=2, num_classes=4))
            eng = eng4
        else:
            eng = eng8
        if eng is eng4:
            # a 4-class handle needs no weights for stage-level calls
            pass
        eng.set_posterior(0, counts, means[:, :, 0], covs, np.zeros(len(counts), np.float32))
        eng._set_centres(0, centres)
        eng.cluster_fuse()
        scores, fmeans, fcovs, fcounts = eng.get_detections(0)
        assert scores.shape == g[t + "_out_scores"].shape
        assert rel_err(fcounts, g[t + "_out_counts"], 1e-6) < 1e-6
        assert rel_err(scores, g[t + "_out_scores"], 1e-6) < REL_TOL
        assert rel_err(fmeans, g[t + "_out_means"][:, :, 0], 1.0) < REL_TOL
        ref_c = g[t + "_out_covs"]
        floor = np.abs(ref_c).reshape(len(ref_c), -1).max(axis=1)[:, None, None] * 1e-2
        assert (np.abs(fcovs - ref_c) / (np.abs(ref_c) + floor)).max() < REL_TOL


def test_clustering_uses_the_callers_affinity_matrix(golden_dir):
    """bayes_od_clustering(..., affinity_matrix, thr) with an affinity that is not the IoU of the means: the device must
    cluster on the caller's matrix (reference :316); expected values = the reference's own outputs (by import).
    The same call with the golden IoU cases' matrices passed explicitly equals the on-the-fly IoU path."""
    import os
    from bayes_od_rc_amd import inference_utils
    g = np.load(os.path.join(golden_dir, "clustering_affinity.npz"))
    thr = float(g["affinity_threshold"])
    for i in range(int(g["n_cases"])):
        t = "a%02d" % i
        s, m, c, k = inference_utils.bayes_od_clustering(g[t + "_counts"], g[t + "_means"], g[t + "_covs"], g[t + "_centres"],
                                                         g[t + "_affinity"], thr)
        assert s.shape == g[t + "_out_scores"].shape and m.shape == g[t + "_out_means"].shape
        assert rel_err(k, g[t + "_out_counts"], 1e-6) < 1e-6
        assert rel_err(s, g[t + "_out_scores"], 1e-6) < REL_TOL
        assert rel_err(m, g[t + "_out_means"], 1.0) < REL_TOL
        ref_c = g[t + "_out_covs"]
        floor = np.abs(ref_c).reshape(len(ref_c), -1).max(axis=1)[:, None, None] * 1e-2
        assert (np.abs(c - ref_c) / (np.abs(ref_c) + floor)).max() < REL_TOL
        # ignoring the matrix (IoU of the means instead) gives different clusters for these cases
    t = "a04"
    s_iou = inference_utils.bayes_od_clustering(g[t + "_counts"], g[t + "_means"], g[t + "_covs"], g[t + "_centres"], None, thr)[0]
    assert rel_err(s_iou, g[t + "_out_scores"], 1e-6) > 1e-2
    gi = np.load(os.path.join(golden_dir, "clustering.npz"))
    t = "c23"
    a = inference_utils.bayes_od_clustering(gi[t + "_counts"], gi[t + "_means"], gi[t + "_covs"], gi[t + "_centres"], gi[t + "_iou"], 0.5)
    b = inference_utils.bayes_od_clustering(gi[t + "_counts"], gi[t + "_means"], gi[t + "_covs"], gi[t + "_centres"], None, 0.5)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    with pytest.raises(ValueError):
        inference_utils.bayes_od_clustering(gi[t + "_counts"], gi[t + "_means"], gi[t + "_covs"], gi[t + "_centres"], gi[t + "_iou"][:5], 0.5)


def _random_posteriors(rng, m, c=8):
    means = np.zeros((m, 4), np.float32)
    means[:, :2] = rng.uniform(10, 90, (m, 2))
    means[:, 2:] = means[:, :2] + rng.uniform(8, 30, (m, 2))
    a = rng.normal(size=(m, 4, 4)).astype(np.float32)
    covs = (a @ a.transpose(0, 2, 1) + 2.0 * np.eye(4, dtype=np.float32)).astype(np.float32)
    counts = (rng.integers(0, 6, (m, c)) + rng.uniform(0.1, 1.0, (m, c))).astype(np.float32)       # Dirichlet-style pseudo counts
    return counts, means, covs


def test_cluster_of_one_member_is_the_member(golden_dir):
    """SURVEY section 4, property: fusing a cluster that holds only its centre returns the centre -- mean unchanged, covariance
    times the calibration constant 70 (inference_utils.py:359-361), normalised counts as score, counts unchanged."""
    rng = np.random.default_rng(3)
    eng, _ = _engine(hw=(128, 128), batch=1, n=2, num_classes=8)
    counts, means, covs = _random_posteriors(rng, 6)
    means[:, :2] += np.arange(6, dtype=np.float32)[:, None] * 200.0          # far apart: every IoU is 0, each box is its own cluster
    means[:, 2:] += np.arange(6, dtype=np.float32)[:, None] * 200.0
    eng.set_posterior(0, counts, means, covs, np.zeros(6, np.float32))
    eng._set_centres(0, np.arange(6, dtype=np.int32))
    eng.cluster_fuse()
    scores, fmeans, fcovs, fcounts = eng.get_detections(0)
    assert scores.shape == (6, 8)
    assert np.allclose(fmeans, means, rtol=1e-4, atol=1e-3)
    assert np.allclose(fcovs, covs * 70.0, rtol=2e-3, atol=1e-3)
    assert np.allclose(fcounts, counts, rtol=1e-6)
    assert np.allclose(scores, counts / counts.sum(axis=1, keepdims=True), rtol=1e-5)


def test_cluster_fuse_is_invariant_to_the_order_of_the_kept_anchors():
    """SURVEY section 4, property: permuting the kept anchors (and re-pointing the centres) must not change a fused detection
    beyond fp32 summation order -- the kernel sums a cluster's precisions over whatever order the members are stored in."""
    rng = np.random.default_rng(11)
    eng, _ = _engine(hw=(128, 128), batch=1, n=2, num_classes=8)
    m = 40
    counts, means, covs = _random_posteriors(rng, m)
    means[: m // 2] = means[0] + rng.normal(0, 1.0, (m // 2, 4)).astype(np.float32)      # one big cluster around box 0
    centres = np.array([0, m - 1, m // 2 + 3], np.int32)
    outs = []
    for trial in range(3):
        perm = np.arange(m) if trial == 0 else rng.permutation(m)
        inv = np.empty(m, np.int64); inv[perm] = np.arange(m)
        eng.set_posterior(0, counts[perm], means[perm], covs[perm], np.zeros(m, np.float32))
        eng._set_centres(0, inv[centres].astype(np.int32))
        eng.cluster_fuse()
        outs.append([x.copy() for x in eng.get_detections(0)])
    for other in outs[1:]:
        assert np.allclose(other[1], outs[0][1], rtol=1e-4, atol=1e-3)       # means
        assert np.allclose(other[2], outs[0][2], rtol=2e-3, atol=1e-3)       # covariances
        # the categorical fusion keeps the three members closest (KL) to the centre: a tie-free top-3 is order-independent
        assert np.allclose(other[0], outs[0][0], rtol=1e-4, atol=1e-6)
        assert np.allclose(other[3], outs[0][3], rtol=1e-5)


def test_iou_matrix_matches_reference_formula(golden_dir):
    import os
    g = np.load(os.path.join(golden_dir, "clustering.npz"))
    eng, _ = _engine(batch=1, n=2)
    t = "c24"
    counts, means, covs = g[t + "_counts"], g[t + "_means"], g[t + "_covs"]
    eng.set_posterior(0, counts, means[:, :, 0], covs, np.zeros(len(counts), np.float32))
    iou = eng.get_iou_matrix(0)
    assert rel_err(iou, g[t + "_iou"], 1e-4) < 1e-5


@pytest.mark.parametrize("dataset", ["bdd", "kitti"])
def test_validation_post_process_matches_oracle(dataset):
    """validation_utils.post_process_predictions (:10-77) on the device: kept set and soft-NMS order exact,
    class rows / corners within 1e-5."""
    from bayes_od_rc_amd import constants, inference_utils
    from bayes_od_rc_amd.anchor_generator import FpnAnchorGenerator
    from conftest import ANCHOR_CFG
    from oracle import validation
    hw = (128, 160)
    anchors = FpnAnchorGenerator(ANCHOR_CFG).generate_all((hw[0], hw[1], 3))
    a = anchors.shape[0]
    rng = np.random.default_rng(3)
    logits = rng.normal(0, 1.5, (1, a, 8)).astype(np.float32)
    logits[..., 7] += 1.0                                         # background wins for most anchors
    box_t = rng.normal(0, 0.6, (1, a, 4)).astype(np.float32)
    sample = {constants.ANCHORS_KEY: anchors[None], constants.IMAGE_NORMALIZED_KEY: np.zeros((1,) + hw + (3,), np.float32),
              constants.ORIGINAL_IM_SIZE_KEY: np.asarray([[375, 1242, 3]], np.int32)}
    pred = {constants.ANCHORS_CLASS_PREDICTIONS_KEY: logits, constants.ANCHORS_BOX_PREDICTIONS_KEY: box_t}
    classes, corners = inference_utils.post_process_predictions(sample, pred, dataset_name=dataset)
    ref_c, ref_b, info = validation.post_process_predictions(anchors, box_t[0], logits[0], dataset_name=dataset, net_hw=hw,
                                                             orig_hw=(375, 1242), dtype=np.float32)
    assert 50 < info["keep"].sum() < a and len(info["nms"]) == 100
    assert classes.shape == ref_c.shape and corners.shape == ref_b.shape
    assert np.abs(classes - ref_c).max() < 1e-5
    assert np.abs(corners - ref_b).max() < 1e-3 * max(1.0, float(np.abs(ref_b).max()))


# ================================================================================================
# Posterior at its configuration corners (post_sample / post_fuse <4> and <8>, every prior pair, no covariance head, the second
# pass of post_fuse_kernel, empty and full kept sets), through BOTH routes: per-sample raw outputs (set_raw + posterior) and the
# statistics record the conv epilogues produce in production (set_statistics + stat_posterior, `aggregated = 1`).
# ================================================================================================
POST_HW = (128, 128)
POST_SEED, POST_FIRST = 987654321987, 11
_NI, _ISO, _NONE = {"type": "non_informative"}, {"type": "isotropic", "isotropic_variance": 100000.0}, {"type": "None"}
# id: (C, N, bg, Dirichlet, Gaussian, covariance head, full covariance, dataset, rng seed, min_checked)
POSTERIOR_ROWS = {
    "c4_kitti_full":        (4, 5, 3.0, _NI, _ISO, True, True, "kitti", 21, 200),
    "c4_none_iso_diagonal": (4, 5, 2.0, _NONE, _ISO, True, False, "bdd", 21, 200),
    "c8_noninf_none":       (8, 5, 3.0, _NI, _NONE, True, True, "bdd", 21, 200),
    "c8_nearly_all_kept":   (8, 5, -3.0, _NI, _ISO, True, True, "bdd", 21, 2049),        # second pass of post_fuse_kernel
    "c4_every_anchor_kept": (4, 5, -20.0, _NONE, _NONE, True, True, "bdd", 21, 3000),
    "c8_nothing_kept":      (8, 5, 30.0, _NONE, _NONE, True, True, "bdd", 21, 0),
    "c8_two_samples":       (8, 2, 3.0, _NI, _ISO, True, True, "bdd", 21, 200),          # rank-1 epistemic covariance
    "c8_no_covar_head":     (8, 16, 3.0, _NI, _ISO, False, True, "bdd", 21, 200),        # likelihood = epistemic / 11
}
KITTI_ORIG = (375, 1242)
_post_cache = {}


def _post_anchors():
    from bayes_od_rc_amd.anchor_generator import FpnAnchorGenerator
    if "anchors" not in _post_cache:
        _post_cache["anchors"] = FpnAnchorGenerator(ANCHOR_CFG).generate_all((POST_HW[0], POST_HW[1], 3))
    return _post_cache["anchors"]


def _oracle_posterior(cls, box, cov, anchors, u, bcfg, full, dataset, dtype):
    from oracle import bayes_od, network
    pred = {"anchors_class_predictions": cls, "anchors_box_predictions": box}
    if cov is not None:
        pred["anchors_box_covar_predictions"] = network.fill_triangular_4(cov)
    kw = dict(dataset_name="kitti", orig_size=KITTI_ORIG + (3,), net_size=POST_HW + (3,)) if dataset == "kitti" else {}
    return bayes_od.bayes_od_posterior(pred, anchors, u, bcfg, use_full_covar=full, dtype=dtype, return_debug=True, **kw)


def _ambiguous(ref, u, eps=1e-5):
    """conftest.compare_posterior's rule: a draw within eps of a CDF boundary may fall either side on the device."""
    cdf = np.cumsum(ref["mean_probs"], axis=1)
    t = u.astype(np.float64) * cdf[:, -1:]
    return np.abs(cdf[:, None, :] - t[:, :, None]).min(axis=(1, 2)) < eps


def _float32_oracle_error(ref, ref32, u):
    """(mean, covariance) error of the float32 oracle against its float64 self, with compare_posterior's floors, on the anchors
    both keep off a CDF boundary: how much of REL_TOL the INPUTS' conditioning uses up before any kernel runs."""
    both = ref["keep"] & ref32["keep"] & ~_ambiguous(ref, u)
    if not both.any():
        return 0.0, 0.0
    i64, i32 = np.cumsum(ref["keep"])[both] - 1, np.cumsum(ref32["keep"])[both] - 1
    e_mean = rel_err(ref32["means"][i32][:, :, 0], ref["means"][i64][:, :, 0], 1.0)
    cov_ref = ref["covs"][i64]
    floor = np.abs(cov_ref).reshape(len(i64), -1).max(axis=1)[:, None, None] * 1e-2
    e_cov = float((np.abs(ref32["covs"][i32] - cov_ref) / (np.abs(cov_ref) + floor)).max())
    return e_mean, e_cov


def _posterior_row(name, batch=2):
    """Inputs and float64 references of one row, computed once and shared by the two routes (never modified)."""
    if name in _post_cache:
        return _post_cache[name]
    from oracle import philox
    c, n, bg, dirichlet, gaussian, head, full, dataset, seed, min_checked = POSTERIOR_ROWS[name]
    anchors = _post_anchors()
    bcfg = {"ranking_method": "score", "dirichlet_prior": dirichlet, "gaussian_prior": gaussian}
    rng = np.random.default_rng(seed)
    cls, box, cov = post_reference.random_raw(rng, batch, n, anchors.shape[0], c=c, bg=bg)
    if not head:
        cov = None
    refs = []
    for img in range(batch):
        u = philox.categorical_uniforms(POST_SEED, POST_FIRST + img, anchors.shape[0])
        args = (cls[img], box[img], None if cov is None else cov[img], anchors, u, bcfg, full, dataset)
        ref = _oracle_posterior(*args, dtype=np.float64)
        guard = _float32_oracle_error(ref, _oracle_posterior(*args, dtype=np.float32), u)
        refs.append((ref, u, guard))
    row = {"c": c, "n": n, "cls": cls, "box": box, "cov": cov, "anchors": anchors, "bcfg": bcfg, "full": full, "dataset": dataset,
           "head": head, "min_checked": min_checked, "refs": refs, "batch": batch}
    _post_cache[name] = row
    return row


def _posterior_engine(row, statistics, bcfg=None, **kw):
    cfgkw = dict(use_full_covar=row["full"], bayes_od_config=bcfg or row["bcfg"], num_classes=row["c"], has_covar_head=row["head"])
    if row["dataset"] == "kitti":
        cfgkw.update(dataset_name="kitti", orig_size=KITTI_ORIG)
    cfgkw.update(kw)
    eng, _ = _engine(hw=POST_HW, batch=row["batch"], n=row["n"], weights=False, mc_statistics=statistics, **cfgkw)
    return eng


def _run_route(eng, row, statistics):
    if statistics:
        rec = post_reference.statistics_record(row["cls"], row["box"], row["cov"], row["anchors"])      # float64, rounded once
        eng.set_statistics(*[None if x is None else x.astype(np.float32) for x in rec], samples=row["n"])
        eng.stat_posterior(seed=POST_SEED, first_image_id=POST_FIRST)
    else:
        eng.set_raw(row["cls"], row["box"], row["cov"])
        eng.posterior(seed=POST_SEED, first_image_id=POST_FIRST)


@pytest.mark.parametrize("route", ["raw", "statistics"])
@pytest.mark.parametrize("name", list(POSTERIOR_ROWS))
def test_posterior_corner_matches_oracle(name, route):
    """Every row of POSTERIOR_ROWS against oracle.bayes_od in float64, counts exact, everything else REL_TOL on every kept anchor
    off a CDF boundary.  Asserted first, from the reference alone: the float32 oracle is within REL_TOL / 4 of the float64 one
    (the inputs are well enough conditioned for a float32 kernel to be held to REL_TOL), and the row keeps what it is there for."""
    row = _posterior_row(name)
    for ref, u, (g_mean, g_cov) in row["refs"]:
        print("%s: float32 oracle mean %.2e covariance %.2e, kept %d, ambiguous %.2f %%"
              % (name, g_mean, g_cov, ref["keep"].sum(), 100 * _ambiguous(ref, u).mean()))
        assert g_mean < REL_TOL / 4 and g_cov < REL_TOL / 4
        assert ref["keep"].sum() >= row["min_checked"]
        if name == "c8_nearly_all_kept":
            assert ref["keep"].sum() > 2048                        # more than POST_FUSE_BLOCKS x 256 slots: the grid stride is taken
        if name == "c4_every_anchor_kept":
            assert ref["keep"].all()
        if name == "c8_nothing_kept":
            assert not ref["keep"].any()
    if name == "c8_nearly_all_kept":
        assert min(ref["keep"].sum() for ref, _, _ in row["refs"]) < 3069       # ... and the compaction still drops an anchor
    eng = _posterior_engine(row, route == "statistics")
    _run_route(eng, row, route == "statistics")
    kept = eng.num_kept()
    for img, (ref, u, _) in enumerate(row["refs"]):
        got = eng.get_posterior(img)
        assert kept[img] == len(got["anchor_index"])
        if name == "c8_nothing_kept":
            assert kept[img] == 0 and got["means"].shape == (0, 4) and got["covs"].shape == (0, 4, 4)
            continue
        checked, same = compare_posterior(got, ref, u, tol=REL_TOL, min_checked=row["min_checked"], max_ambiguous=2e-2,
                                          boundary_eps=1e-5)
        if same:
            assert kept[img] == ref["keep"].sum()
        gi = np.searchsorted(got["anchor_index"], np.nonzero(ref["keep"] & ~_ambiguous(ref, u))[0])
        ri = np.cumsum(ref["keep"])[ref["keep"] & ~_ambiguous(ref, u)] - 1
        cov_ref = ref["covs"][ri]                                  # (the figures compare_posterior has just asserted, for the log)
        floor = np.abs(cov_ref).reshape(len(ri), -1).max(axis=1)[:, None, None] * 1e-2
        print("%s/%s image %d: %d anchors compared, errors: score %.2e mean %.2e covariance %.2e ranking %.2e (bound %.0e)"
              % (name, route, img, checked, rel_err(got["score"][gi], ref["score"][ri], 1e-6),
                 rel_err(got["means"][gi], ref["means"][ri][:, :, 0], 1.0),
                 float((np.abs(got["covs"][gi] - cov_ref) / (np.abs(cov_ref) + floor)).max()),
                 rel_err(got["ranking"][gi], ref["ranking"][ri], 1e-6), REL_TOL))
        assert rel_err(got["ranking"][gi], ref["ranking"][ri], 1e-6) < REL_TOL           # ranking_method 'score'
        c = got["covs"]
        assert np.allclose(c, np.transpose(c, (0, 2, 1)), rtol=1e-5, atol=1e-7)
    if name == "c8_nothing_kept":                                  # the later stages run on empty images and return nothing
        eng.nms()
        eng.cluster_fuse()
        for img in range(row["batch"]):
            assert eng.get_nms(img).shape == (0,)
            s, m, cv, k = eng.get_detections(img)
            assert s.shape == (0, 8) and m.shape == (0, 4) and cv.shape == (0, 4, 4) and k.shape == (0, 8)


# ================================================================================================
# Joint-entropy ranking (joint_entropy_kernel) at its corners
# ================================================================================================
_JE_CFG = {"ranking_method": "joint_entropy", "dirichlet_prior": _NI, "gaussian_prior": _ISO}
ONE_KEPT_ANCHOR = 1234
# id: (C, full covariance, dataset, batch, rng seed)
JE_CASES = {
    "c4_kitti_full": (4, True, "kitti", 1, 21),              # the reference's kitti_entropy configuration: ranked on the rescaled covariances
    "c8_diagonal": (8, False, "bdd", 1, 23),
    "empty_first_image": (8, True, "bdd", 2, 23),            # the min-max is per image: an empty image 0 must not disturb image 1
    "one_kept_anchor": (8, True, "bdd", 1, 21),              # M = 1: both min-max denominators clamp
}


def _je_case(name):
    key = "je_" + name
    if key in _post_cache:
        return _post_cache[key]
    from oracle import philox
    c, full, dataset, batch, seed = JE_CASES[name]
    anchors = _post_anchors()
    rng = np.random.default_rng(seed)
    cls, box, cov = post_reference.random_raw(rng, batch, 5, anchors.shape[0], c=c, bg=30.0 if name == "one_kept_anchor" else 3.0)
    if name == "empty_first_image":
        cls[0, :, :, -1] += 27.0                                  # bg = +30 on image 0
    if name == "one_kept_anchor":
        cls[0, :, ONE_KEPT_ANCHOR, -1] -= 30.0
        cls[0, :, ONE_KEPT_ANCHOR, 2] += 40.0                     # a +40 foreground logit in every sample
    refs = []
    for img in range(batch):
        u = philox.categorical_uniforms(POST_SEED, POST_FIRST + img, anchors.shape[0])
        empty = name == "empty_first_image" and img == 0          # (the oracle's min() has nothing to reduce: 'score' gives the kept set)
        bcfg = dict(_JE_CFG, ranking_method="score") if empty else _JE_CFG
        refs.append((_oracle_posterior(cls[img], box[img], cov[img], anchors, u, bcfg, full, dataset, np.float64), u))
    row = {"c": c, "n": 5, "cls": cls, "box": box, "cov": cov, "anchors": anchors, "bcfg": _JE_CFG, "full": full, "dataset": dataset,
           "head": True, "refs": refs, "batch": batch}
    _post_cache[key] = row
    return row


def _keep_is_robust(ref, u):
    """No anchor on a CDF boundary can change sides of the background filter by moving one draw to a neighbouring class: the
    kept sets of device and oracle are then identical, and the min-max normalised ranking is comparable on all of it."""
    s = ref["samples"]
    d = (s[:, -1] - s[:, :-1].max(axis=1))[_ambiguous(ref, u)]
    return bool(np.all(np.abs(d) > 2))


@pytest.mark.parametrize("route", ["raw", "statistics"])
@pytest.mark.parametrize("name", list(JE_CASES))
def test_joint_entropy_ranking_corner(name, route):
    """got['ranking'] against the oracle's min-max normalised information gains (floor 1e-2, REL_TOL), on identical kept sets --
    which the reference alone guarantees here (_keep_is_robust)."""
    row = _je_case(name)
    for ref, u in row["refs"]:
        assert _keep_is_robust(ref, u)
    eng = _posterior_engine(row, route == "statistics")
    _run_route(eng, row, route == "statistics")
    kept = eng.num_kept()
    for img, (ref, u) in enumerate(row["refs"]):
        got = eng.get_posterior(img)
        got_keep = np.zeros(len(ref["keep"]), bool)
        got_keep[got["anchor_index"]] = True
        assert np.array_equal(got_keep, ref["keep"]) and kept[img] == ref["keep"].sum()
        if name == "empty_first_image" and img == 0:
            assert kept[img] == 0
            continue
        if name == "one_kept_anchor":
            assert kept[img] == 1 and got["anchor_index"][0] == ONE_KEPT_ANCHOR
            assert ref["ranking"].shape == (1,) and ref["ranking"][0] == 0.0
            assert got["ranking"][0] == 0.0                        # 0 / max(1, 0) + 0 / max(0.001, 0), exactly
            continue
        assert kept[img] >= 200
        err = rel_err(got["ranking"], ref["ranking"], 1e-2)
        print("%s/%s image %d: %d boxes ranked, error %.2e" % (name, route, img, kept[img], err))
        assert err < REL_TOL
        compare_posterior(got, ref, u, tol=REL_TOL, min_checked=200)


# ================================================================================================
# Soft-NMS at the storage switches of nms_kernel and beyond the default configuration: index lists stay bit-exact
# ================================================================================================
def _nms_inputs(seed, sizes, ties=True):
    """Per image (corners, ranking) of `_posterior_like` boxes; image 1 carries the half-the-scores-tied pattern."""
    rng = np.random.default_rng(seed)
    out = []
    for img, (m, n_obj) in enumerate(sizes):
        counts, means, covs, ranking = _posterior_like(rng, m, n_obj)
        if ties and img == 1:
            ranking[: m // 2] = ranking[0]
        out.append((counts, means, covs, ranking))
    return out


def _check_nms(inputs, variant, max_out=100, sigma=0.5, thr=0.5):
    from oracle import nms, geometry
    eng, _ = _engine(hw=(256, 256), batch=2, n=2, weights=False, nms_variant=variant,
                     nms_config={"max_output_size": max_out, "iou_threshold": thr, "soft_nms_sigma": sigma})
    for img, (counts, means, covs, ranking) in enumerate(inputs):
        eng.set_posterior(img, counts, means, covs, ranking)
    eng.nms()
    refs = []
    for img, (counts, means, covs, ranking) in enumerate(inputs):
        ref_idx, _ = nms.soft_nms(geometry.vuhw_to_vuvu(means), ranking, max_out, thr, sigma, variant=variant)
        got = eng.get_nms(img)
        assert np.array_equal(got, ref_idx), (img, len(got), len(ref_idx), got[:10], ref_idx[:10])
        refs.append(ref_idx)
    return refs


@pytest.mark.parametrize("variant", ["A", "B"])
@pytest.mark.parametrize("m0,m1", [(64, 65), (512, 513), (4096, 4097), (6144, 6145)])
def test_soft_nms_at_the_storage_switches(variant, m0, m1):
    """One wave's stride (64), the -inf padding (512), boxes in LDS or in HBM (NMS_BOX_CAP = 4096), scores in LDS or in the
    per-image workspace (NMS_LDS_CAP = 6144): M on the switch in image 0 and one past it in image 1 of the same launch, so the
    two images also take different storage side by side."""
    refs = _check_nms(_nms_inputs(m0, [(m0, max(2, m0 // 12)), (m1, max(2, m1 // 12))]), variant)
    assert all(len(r) == min(100, m) for r, m in zip(refs, (m0, m1)))


@pytest.mark.parametrize("variant", ["A", "B"])
@pytest.mark.parametrize("max_out", [1, 65, 512])
def test_soft_nms_max_output_size(variant, max_out):
    """65 and 512 selected boxes take the decay loop through more than one chunk of 64; 512 is NMS_MAX_OUT."""
    refs = _check_nms(_nms_inputs(700 + max_out, [(700, 300), (700, 300)]), variant, max_out=max_out)
    assert all(len(r) == max_out for r in refs)


@pytest.mark.parametrize("variant", ["A", "B"])
def test_soft_nms_sigma_zero_is_hard_nms(variant):
    """soft_nms_sigma = 0 on the 37-box / 3-object case.  Variant A (TF 2.0-2.2) multiplies a suppressed score by 0 and re-queues
    it (score 0 > -inf), so all 37 boxes come out, 34 of them behind the survivors; variant B (TF >= 2.3) drops a box over the
    IoU threshold for good and returns the 3 survivors."""
    refs = _check_nms(_nms_inputs(37, [(37, 3), (37, 3)]), variant, sigma=0.0)
    assert [len(r) for r in refs] == ([37, 37] if variant == "A" else [3, 3])


@pytest.mark.parametrize("variant", ["A", "B"])
@pytest.mark.parametrize("sigma", [0.5, 0.0])
def test_soft_nms_degenerate_boxes(variant, sigma):
    """Zero-area boxes (IoU 0 with everything, themselves included), corners in the wrong order (the op sorts them), ten exact
    duplicates with equal scores (lowest index first, the other nine decayed or suppressed), half the scores tied."""
    inputs = _nms_inputs(101, [(100, 12), (101, 12)])
    for img, (counts, means, covs, ranking) in enumerate(inputs):
        means[3:6, 2] = 0.0                                        # zero height
        means[8, 3] = 0.0                                          # zero width
        means[9, 2:] = 0.0                                         # a point
        means[12:15, 2] *= -1.0                                    # y1 > y2
        means[16, 2:] *= -1.0                                      # both pairs swapped
        means[40:50] = means[40]
        ranking[40:50] = ranking[40] if img == 0 else ranking[0]   # image 1: the duplicates sit inside the tied half
    refs = _check_nms(inputs, variant, sigma=sigma)
    assert all(len(r) >= 12 for r in refs)


# ================================================================================================
# cluster_fuse_kernel against oracle/clustering.py in float64 on the same float32-valued inputs
# ================================================================================================
def _clustered_posteriors(rng, sizes, c, singles=0, distractors=2, counts="continuous"):
    """Boxes in clusters of the given sizes on a wide canvas (cell k holds cluster k: members jittered by a pixel around the
    cluster's first box, IoU ~ 0.9; `distractors` boxes per cluster shifted by 0.45 of its height, IoU ~ 0.4), plus `singles`
    boxes alone in their cells; all shuffled, so a cluster's members fall on the threads of the block in no order.
    Returns counts [m,c], means [m,4] (v,u,h,w), covs [m,4,4], float32, and the index of each cluster's first box."""
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
    if counts == "continuous":                                     # Dirichlet-style pseudo counts: no two rows alike, no KL ties
        cnt = rng.integers(0, 6, (m, c)) + rng.uniform(0.1, 1.0, (m, c))
    else:                                                          # raw multinomial counts, no prior added: exact zeros
        cnt = np.stack([rng.multinomial(30, p) for p in rng.dirichlet(np.ones(c) * 0.5, size=m)]).astype(np.float64)
    return cnt.astype(np.float32), means, covs, inv[np.asarray(first)][:len(sizes)].astype(np.int32)


def _cluster_reference(counts, means, covs, centres, affinity=None, thr=0.5, ties=()):
    """oracle.clustering on the float32 values in float64, with the guards that make a float32 kernel comparable to it: no member
    within 1e-4 of the threshold; the gap between the third and the fourth smallest KL above 1e-4 unless the tie is exact and
    meant (`ties`: 'zero' = duplicated count rows, 'inf' = rows of infinite KL, taken by lowest index on both sides)."""
    from oracle import clustering, geometry
    if affinity is None:
        affinity = post_reference.iou_plus1(geometry.vuhw_to_vuvu(means))          # the corners the device holds, IoU in float64
    cols = affinity[:, centres]
    assert np.abs(cols - thr).min() > 1e-4
    with np.errstate(invalid="ignore"):                            # (the margin between two infinite KLs is inf - inf)
        out = clustering.bayes_od_clustering(counts.astype(np.float64), means.astype(np.float64)[:, :, None],
                                             covs.astype(np.float64), centres, affinity, thr, return_margins=True)
    margins = out[4]
    ok = margins > 1e-4
    if "zero" in ties:
        ok |= margins == 0.0
    if "inf" in ties:
        ok |= np.isnan(margins)                                    # inf - inf: the top three reach into the rows of infinite KL
    assert ok.all(), margins
    return out, (cols > thr).sum(axis=0)


def _compare_clusters(det, ref):
    scores, fmeans, fcovs, fcounts = det
    r_scores, r_means, r_covs, r_counts = ref[:4]
    assert scores.shape == r_scores.shape and fmeans.shape == r_means[:, :, 0].shape and fcovs.shape == r_covs.shape
    floor = np.abs(r_covs).reshape(len(r_covs), -1).max(axis=1)[:, None, None] * 1e-2
    errs = (rel_err(fcounts, r_counts, 1e-6), rel_err(scores, r_scores, 1e-6), rel_err(fmeans, r_means[:, :, 0], 1.0),
            float((np.abs(fcovs - r_covs) / (np.abs(r_covs) + floor)).max()))
    print("clusters: counts %.1e scores %.1e means %.1e covariances %.1e" % errs)
    # counts and scores are fp32 sums of at most three rows (the float32 oracle is within 1e-7 of the float64 one): 1e-5 relative
    assert errs[0] < 1e-5 and errs[1] < 1e-5
    assert errs[2] < REL_TOL and errs[3] < REL_TOL
    return errs


def _cluster_engine(c, batch=1):
    return _engine(hw=(128, 128), batch=batch, n=2, weights=False, num_classes=c)[0]


def _run_clusters(eng, img, counts, means, covs, centres):
    eng.set_posterior(img, counts, means, covs, np.zeros(len(counts), np.float32))
    eng._set_centres(img, centres)


@pytest.mark.parametrize("c", [4, 8])
@pytest.mark.parametrize("sizes", [(1, 2, 3, 4), (255, 256, 257)], ids=["sizes_1_2_3_4", "sizes_255_256_257"])
def test_cluster_fuse_sizes_match_oracle(c, sizes):
    """Clusters of one to four members (the `total <= 3` switch between averaging all members and the three closest in KL) and of
    255 / 256 / 257 members (one block stride of 256 threads and its wrap)."""
    rng = np.random.default_rng(10 * c + len(sizes))
    counts, means, covs, centres = _clustered_posteriors(rng, sizes, c, singles=5)
    ref, members = _cluster_reference(counts, means, covs, centres)
    assert tuple(members) == tuple(sizes)
    eng = _cluster_engine(c)
    _run_clusters(eng, 0, counts, means, covs, centres)
    eng.cluster_fuse()
    _compare_clusters(eng.get_detections(0), ref)


@pytest.mark.parametrize("c", [4, 8])
def test_cluster_fuse_large_image_matches_oracle(c):
    """M = 1500 boxes, one cluster holding a third of them (every thread of the block fuses two members), three small ones."""
    rng = np.random.default_rng(1500 + c)
    counts, means, covs, centres = _clustered_posteriors(rng, (500, 7, 2, 1), c, singles=1500 - 510 - 8)
    assert len(counts) == 1500
    ref, members = _cluster_reference(counts, means, covs, centres)
    assert tuple(members) == (500, 7, 2, 1)
    eng = _cluster_engine(c)
    _run_clusters(eng, 0, counts, means, covs, centres)
    eng.cluster_fuse()
    _compare_clusters(eng.get_detections(0), ref)


@pytest.mark.parametrize("c", [4, 8])
def test_cluster_fuse_hundred_centres_on_the_second_image(c):
    """K = 100 centres (the whole grid row of an image) on image 1 of a batch-2 handle, another M and K on image 0."""
    rng = np.random.default_rng(100 + c)
    sizes1 = tuple(int(s) for s in rng.integers(1, 7, 100))
    img0 = _clustered_posteriors(rng, (5, 3, 9), c, singles=20)
    img1 = _clustered_posteriors(rng, sizes1, c, singles=10)
    assert len(img0[0]) != len(img1[0]) and len(img1[3]) == 100
    refs = [_cluster_reference(*x) for x in (img0, img1)]
    assert tuple(refs[1][1]) == sizes1
    eng = _cluster_engine(c, batch=2)
    _run_clusters(eng, 0, *img0)
    _run_clusters(eng, 1, *img1)
    eng.cluster_fuse()
    for img in range(2):
        _compare_clusters(eng.get_detections(img), refs[img][0])


@pytest.mark.parametrize("c", [4, 8])
def test_cluster_fuse_counts_with_exact_zeros(c):
    """Integer counts with no prior added: a member with a zero where the centre has none is at infinite KL, all such members tie,
    and the top three are filled up by lowest index (the oracle's stable sort).  The centres' own rows have no zero."""
    rng = np.random.default_rng(40 + c)
    sizes = (12, 6, 4, 9)
    counts, means, covs, centres = _clustered_posteriors(rng, sizes, c, singles=3, counts="multinomial")
    for k in centres:
        counts[k] = np.float32(30 // c) + np.arange(c, dtype=np.float32) % 2      # every class seen
    assert (counts == 0).any(axis=1).mean() > 0.5
    ref, members = _cluster_reference(counts, means, covs, centres, ties=("inf",))
    assert tuple(members) == sizes and np.isnan(ref[4]).any()       # at least one cluster's top three reach into the infinite rows
    eng = _cluster_engine(c)
    _run_clusters(eng, 0, counts, means, covs, centres)
    eng.cluster_fuse()
    _compare_clusters(eng.get_detections(0), ref)


@pytest.mark.parametrize("c", [4, 8])
def test_cluster_fuse_duplicated_count_rows_tie_exactly(c):
    """Three members carry the centre's count row: four rows at KL = 0 compete for three places.  Whichever three win, the result
    is the same -- but a selection that drops or repeats a row on a tie is not."""
    rng = np.random.default_rng(70 + c)
    sizes = (7, 5, 9)
    counts, means, covs, centres = _clustered_posteriors(rng, sizes, c, singles=4)
    from oracle import geometry
    iou = post_reference.iou_plus1(geometry.vuhw_to_vuvu(means))
    for k in centres:
        others = np.nonzero((iou[:, k] > 0.5) & (np.arange(len(counts)) != k))[0]
        counts[others[-3:]] = counts[k]                             # the three members of highest index
    ref, members = _cluster_reference(counts, means, covs, centres, ties=("zero",))
    assert tuple(members) == sizes and np.all(ref[4] == 0.0)
    eng = _cluster_engine(c)
    _run_clusters(eng, 0, counts, means, covs, centres)
    eng.cluster_fuse()
    _compare_clusters(eng.get_detections(0), ref)


@pytest.mark.parametrize("c", [4, 8])
def test_cluster_fuse_on_a_callers_affinity_large_image(c):
    """bod_set_affinity at M = 1500 with a matrix that is not the IoU: membership follows the caller's columns."""
    from oracle import geometry
    rng = np.random.default_rng(900 + c)
    counts, means, covs, centres = _clustered_posteriors(rng, (40, 30, 20, 10, 5), c, singles=1500 - 105 - 10)
    m = len(counts)
    assert m == 1500
    cols = rng.random((len(centres), m))
    cols = np.where(cols > 0.5, cols + 0.01, cols - 0.01).astype(np.float32)          # nothing near the threshold
    cols[:, :] = np.where(rng.random(cols.shape) < 0.9, np.minimum(cols, 0.2), cols)  # ~5 % members: a different set per centre
    affinity = np.zeros((m, m), np.float32)
    affinity[:, centres] = cols.T
    ref, members = _cluster_reference(counts, means, covs, centres, affinity=affinity.astype(np.float64))
    iou_members = (post_reference.iou_plus1(geometry.vuhw_to_vuvu(means))[:, centres] > 0.5).sum(axis=0)
    assert members.min() > 3 and not np.array_equal(members, iou_members)
    eng = _cluster_engine(c)
    _run_clusters(eng, 0, counts, means, covs, centres)
    eng.set_affinity(0, cols)
    eng.cluster_fuse()
    _compare_clusters(eng.get_detections(0), ref)
