"""Covariance parts, host side: the float64 restatement (tests/cov_parts_reference.py) against the oracle it decomposes, and the
feature's surface that needs no GPU -- the ABI symbols, the config field, the wide record row, the writer's directories."""
import ctypes
import os
import re

import numpy as np
import pytest

import cov_parts_reference as cpr
import post_reference
from conftest import ANCHOR_CFG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARTS_SYMBOLS = ["bod_get_posterior_parts", "bod_set_posterior_parts", "bod_get_detection_parts", "bod_get_detection_parts_batch",
                 "bod_collect_parts", "bod_device_detection_parts"]
_NI = {"type": "non_informative"}


def _gauss(iso):
    return {"type": "None"} if iso is None else {"type": "isotropic", "isotropic_variance": float(iso)}


@pytest.fixture(scope="module")
def raw_case():
    """One image of the posterior tests' random head outputs at 128 x 128 (A = 3 069, N = 5) and its categorical uniforms."""
    from bayes_od_rc_amd.anchor_generator import FpnAnchorGenerator
    from oracle import network, philox
    anchors = FpnAnchorGenerator(ANCHOR_CFG).generate_all((128, 128, 3))
    cls, box, cov = post_reference.random_raw(np.random.default_rng(21), 1, 5, anchors.shape[0])
    pred = {"anchors_class_predictions": cls[0], "anchors_box_predictions": box[0],
            "anchors_box_covar_predictions": network.fill_triangular_4(cov[0])}
    return anchors, pred, philox.categorical_uniforms(987654321987, 11, anchors.shape[0])


@pytest.mark.parametrize("use_full_covar", [True, False])
@pytest.mark.parametrize("iso", [1e5, 50.0, 5.0, None])
@pytest.mark.parametrize("dataset", ["bdd", "kitti"])
def test_restated_parts_sum_to_the_oracles_posterior_covariance(raw_case, dataset, iso, use_full_covar):
    """Pins the reference, not the feature: epi + ale + pri equals oracle.bayes_od's covs within 1e-12 of the largest entry."""
    from oracle import bayes_od
    anchors, pred, u = raw_case
    bcfg = {"ranking_method": "score", "dirichlet_prior": _NI, "gaussian_prior": _gauss(iso)}
    kitti = dict(dataset_name="kitti", orig_size=(375, 1242, 3), net_size=(128, 128, 3)) if dataset == "kitti" else {}
    ref = bayes_od.bayes_od_posterior(pred, anchors, u, bcfg, use_full_covar=use_full_covar, dtype=np.float64, return_debug=True, **kitti)
    scale = cpr.kitti_scale((375, 1242), (128, 128)) if dataset == "kitti" else None
    parts = cpr.posterior_parts(ref, bcfg, scale=scale)
    assert parts.shape == (len(ref["covs"]), 3, 4, 4) and len(parts) > 100
    err = np.abs(parts.sum(axis=1) - ref["covs"]).reshape(len(parts), -1).max(axis=1) / np.abs(ref["covs"]).reshape(len(parts), -1).max(axis=1)
    assert err.max() < 1e-12, float(err.max())
    assert np.abs(parts - np.transpose(parts, (0, 1, 3, 2))).max() < 1e-12 * np.abs(ref["covs"]).max()
    if iso is None:
        assert not parts[:, 2].any()
    else:
        assert np.all(np.linalg.eigvalsh(parts[:, 2]) > 0)
    # the prior's share of the trace: negligible at the suite's 1e5, dominant at 5 (why the GPU tests use the small variances too)
    share = np.trace(parts[:, 2], axis1=1, axis2=2) / np.trace(ref["covs"], axis1=1, axis2=2)
    if iso == 1e5 and dataset == "bdd":
        assert share.max() < 1e-3
    if iso == 5.0 and dataset == "bdd":
        assert share.max() > 0.1


def test_restated_parts_without_a_covariance_head_have_no_aleatoric_term(raw_case):
    from oracle import bayes_od
    anchors, pred, u = raw_case
    pred = {k: v for k, v in pred.items() if k != "anchors_box_covar_predictions"}
    bcfg = {"ranking_method": "score", "dirichlet_prior": _NI, "gaussian_prior": _gauss(5.0)}
    ref = bayes_od.bayes_od_posterior(pred, anchors, u, bcfg, dtype=np.float64, return_debug=True)
    parts = cpr.posterior_parts(ref, bcfg)
    assert not parts[:, 1].any()
    # Without the head lik = E / 11 is the sample covariance of 5 boxes alone (4 degrees of freedom for a 4x4 matrix): its condition
    # number reaches 1e8, and the oracle's covs and the restatement's P each come out of two float64 inversions of it, good to
    # cond * eps apiece.  The identity is therefore held to 8 cond(lik) eps per row -- four inversions, a factor 2 for the products.
    n = len(parts)
    err = np.abs(parts.sum(axis=1) - ref["covs"]).reshape(n, -1).max(axis=1) / np.abs(ref["covs"]).reshape(n, -1).max(axis=1)
    bound = 8.0 * np.linalg.cond(ref["cov_lik"]) * np.finfo(np.float64).eps
    assert np.all(err < bound), float((err / bound).max())


def test_restated_cluster_parts_sum_to_the_oracles_fused_covariance(raw_case):
    """... and the same for oracle.clustering.bayes_od_clustering's output covariance (70 F), membership by its rule."""
    from oracle import bayes_od, clustering
    anchors, pred, u = raw_case
    bcfg = {"ranking_method": "score", "dirichlet_prior": _NI, "gaussian_prior": _gauss(50.0)}
    ref = bayes_od.bayes_od_posterior(pred, anchors, u, bcfg, use_full_covar=True, dtype=np.float64, return_debug=True)
    parts = cpr.posterior_parts(ref, bcfg)
    m = len(parts)
    aff = post_reference.iou_plus1(ref["corners"])
    centres = np.arange(0, m, 17)
    sizes = (aff[:, centres] > 0.5).sum(axis=0)
    assert sizes.min() >= 1 and sizes.max() > 3
    _, _, fcovs, _ = clustering.bayes_od_clustering(ref["counts"], ref["means"], ref["covs"], centres, aff, 0.5)
    got = cpr.cluster_parts(ref["covs"], parts, centres, aff, 0.5)
    assert got.shape == (len(centres), 3, 4, 4)
    err = np.abs(got.sum(axis=1) - fcovs).reshape(len(got), -1).max(axis=1) / np.abs(fcovs).reshape(len(got), -1).max(axis=1)
    assert err.max() < 1e-12, float(err.max())
    # a cluster of one member returns the member's parts times the calibration constant
    one = np.nonzero(sizes == 1)[0]
    if len(one):
        assert np.allclose(got[one[0]], clustering.COV_CALIBRATION * parts[centres[one[0]]], rtol=1e-9)


def test_parts_symbols_in_header_binding_cdef_and_library():
    from bayes_od_rc_amd import _lib, build
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bayesod.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(bod_[a-z0-9_]+)\s*\(", header))
    cdef = set(re.findall(r"\b(bod_[a-z0-9_]+)\s*\(", build.cdef_text()))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in PARTS_SYMBOLS:
        assert name in declared and name in cdef and name in _lib.SIGNATURES, name
        assert getattr(lib, name) is not None
    assert set(_lib.SIGNATURES) == declared
    assert open(os.path.join(ROOT, "include", "bayesod_cdef.h")).read() == build.cdef_text()
    # the field took the last reserved int: the size and the offsets in front of it are unchanged
    assert ctypes.sizeof(_lib.BodConfig) == 31 * 4
    assert _lib.BodConfig.covariance_parts.offset == 30 * 4 and _lib.BodConfig.mc_statistics.offset == 29 * 4
    assert re.search(r"int32_t\s+covariance_parts;", header)


def test_make_config_translates_covariance_parts():
    from bayes_od_rc_amd.engine import make_config
    assert make_config((128, 128)).covariance_parts == 0
    assert make_config((128, 128), covariance_parts=True).covariance_parts == 1
    assert make_config((128, 128), mc_samples=3, mc_ensemble_size=12, mc_statistics=True, covariance_parts=True).covariance_parts == 1
    with pytest.raises(ValueError, match="covariance_parts"):
        make_config((128, 128), mc_samples=1, training=True, covariance_parts=True)


def test_wide_record_round_trip():
    import torch
    from bayes_od_rc_amd import distributed as bd
    rng = np.random.default_rng(2)
    b, k, c = 3, 7, 8
    num = np.array([0, 4, 7], np.int32)
    scores, counts = rng.random((b, k, c), np.float32), rng.random((b, k, c), np.float32)
    means, covs = rng.random((b, k, 4), np.float32), rng.random((b, k, 4, 4), np.float32)
    parts = rng.random((b, k, 3, 4, 4), np.float32)
    t = [torch.from_numpy(x) for x in (num, scores, means, covs, counts)]
    narrow = bd.pack_records(*t)
    wide = bd.pack_records(*t, cov_parts=torch.from_numpy(parts))
    assert narrow.shape == (b, k, bd.record_width(c)) and bd.record_width(c) == 21 + 2 * c
    assert wide.shape == (b, k, bd.record_width(c, cov_parts=True)) and bd.record_width(c, cov_parts=True) == 21 + 2 * c + 48
    assert np.array_equal(wide[:, :, :21 + 2 * c].numpy(), narrow.numpy())
    for img, row in enumerate(bd.unpack_records(wide, c)):
        n = int(num[img])
        assert len(row) == 5 and row[4].shape == (n, 3, 4, 4)
        assert np.array_equal(row[4], parts[img, :n]) and np.array_equal(row[2], covs[img, :n]) and np.array_equal(row[3], counts[img, :n])
        assert not wide[img, n:].numpy().any()                 # zero beyond the image's count, parts included
    assert all(len(row) == 4 for row in bd.unpack_records(narrow, c))
    with pytest.raises(ValueError):
        bd.unpack_records(wide[:, :, :-1], c)


def test_writer_creates_the_part_directories_only_when_asked(tmp_path):
    from bayes_od_rc_amd import writers
    k = 3
    args = (np.zeros((k, 4)), np.full((k, 8), 0.125), np.zeros((k, 4)), np.zeros((k, 4, 4)), np.full((k, 8), 0.125), np.ones((k, 8)), ["car"] * 7)
    plain = writers.PredictionWriter(str(tmp_path / "plain"), "bdd", 1)
    plain.write("000000", *args)
    assert sorted(os.listdir(plain.root)) == ["cat_count", "cat_param", "cov", "data", "mean"]       # the reference layout, as ever
    parts = np.arange(k * 48, dtype=np.float32).reshape(k, 3, 4, 4)
    wide = writers.PredictionWriter(str(tmp_path / "wide"), "bdd", 1, cov_parts=True)
    wide.write("000000", *args, output_cov_parts=parts)
    assert sorted(os.listdir(wide.root)) == ["cat_count", "cat_param", "cov", "cov_aleatoric", "cov_epistemic", "cov_prior", "data", "mean"]
    for i, name in enumerate(("cov_epistemic", "cov_aleatoric", "cov_prior")):
        got = np.load(os.path.join(wide.root, name, "000000.npy"))
        assert got.shape == (k, 4, 4) and np.array_equal(got, parts[:, i])
    with pytest.raises(ValueError):
        wide.write("000001", *args)
