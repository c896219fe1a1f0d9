"""Host-side checks of black-box MC dropout (no GPU): the float64 restatement on a pool computed by hand, the
conditions its generator asserts, flag / yaml precedence, the tree's name, the refusals made before anything is built, and the
presence of the new entry points in the ctypes table and the header."""
import argparse
import os

import numpy as np
import pytest

import blackbox_reference as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _det(score_row, mean, cov_diag):
    return np.asarray(score_row, np.float32), np.asarray(mean, np.float32), np.diag(np.asarray(cov_diag, np.float32))


def _samples(per_sample, c=4):
    out = []
    for dets in per_sample:
        out.append({"scores": np.array([d[0] for d in dets], np.float32).reshape(-1, c),
                    "means": np.array([d[1] for d in dets], np.float32).reshape(-1, 4),
                    "covs": np.array([d[2] for d in dets], np.float32).reshape(-1, 4, 4)})
    return out


def test_two_member_pool_by_hand():
    """Two overlapping boxes from two samples and one box far away.  Centre = the 0.75 box (sample 1); d = (-2, 2, 0, 4)."""
    a = _det([0.5, 0.25, 0.125, 0.125], [100, 100, 40, 40], [1, 1, 1, 1])
    b = _det([0.75, 0.125, 0.0625, 0.0625], [102, 98, 40, 36], [3, 3, 3, 3])
    far = _det([0.125, 0.625, 0.125, 0.125], [300, 300, 20, 20], [2, 2, 2, 2])
    ref = br.pool_merge_reference(_samples([[a, far], [b]]), kmax=10)
    assert list(ref["members"]) == [2, 1]
    assert list(ref["centre"]) == [10, 1]                      # pooled index n * Kmax + rank
    assert np.array_equal(ref["means"][0], [101.0, 99.0, 40.0, 38.0])
    assert np.array_equal(ref["within"][0], np.diag([2.0] * 4))
    d = np.array([-2.0, 2.0, 0.0, 4.0])
    # sum d d^T - 2 dbar dbar^T = d d^T / 2, over n - 1 = 1
    assert np.allclose(ref["between"][0], np.outer(d, d) / 2.0, rtol=0, atol=1e-12)
    assert np.allclose(ref["covs"][0], np.diag([2.0] * 4) + np.outer(d, d) / 2.0, rtol=0, atol=1e-12)
    assert np.array_equal(ref["counts"][0], [1.25, 0.375, 0.1875, 0.1875])
    assert np.array_equal(ref["scores"][0], [0.625, 0.1875, 0.09375, 0.09375])
    # the single member: its own row, between exactly zero
    assert np.array_equal(ref["means"][1], far[1]) and np.array_equal(ref["covs"][1], far[2])
    assert not ref["between"][1].any() and np.array_equal(ref["scores"][1], far[0])
    for key in ("means", "covs", "between", "scores"):
        assert (ref["bound"][key][0] > 0).any() and ref["bound"][key].shape == ref[key].shape
    assert not ref["bound"]["between"][1].any()


def test_min_members_consumes_and_kmax_truncates():
    a = _det([0.5, 0.25, 0.125, 0.125], [100, 100, 40, 40], [1, 1, 1, 1])
    b = _det([0.75, 0.125, 0.0625, 0.0625], [102, 98, 40, 36], [3, 3, 3, 3])
    far = _det([0.125, 0.625, 0.125, 0.125], [300, 300, 20, 20], [2, 2, 2, 2])
    ref = br.pool_merge_reference(_samples([[a, far], [b]]), kmax=10, min_members=2)
    assert list(ref["members"]) == [2] and list(ref["centre"]) == [10]
    other = _det([0.25, 0.375, 0.25, 0.125], [500, 500, 20, 20], [2, 2, 2, 2])
    ref = br.pool_merge_reference(_samples([[a, far], [b, other]]), kmax=2)          # three clusters, two rows
    assert list(ref["members"]) == [2, 1] and list(ref["centre"]) == [2, 1]
    ref = br.pool_merge_reference(_samples([[], []]), kmax=10)
    assert ref["members"].shape == (0,) and ref["covs"].shape == (0, 4, 4) and ref["scores"].shape == (0, 4)


def test_generator_satisfies_its_conditions_and_builds_the_clusters():
    rng = np.random.default_rng(0)
    clusters = [[0], [0, 1], [0, 1, 2], [1, 1], [2] * 30 + [0] * 30]
    samples = br.clustered_pool(rng, clusters, 8, 3, 100)
    br.check_pool_conditions(samples, 100, 0.5)
    ref = br.pool_merge_reference(samples, 100)
    assert sorted(ref["members"]) == sorted(len(cl) for cl in clusters)
    assert np.all(np.diff([samples[c // 100]["scores"][c % 100].max() for c in ref["centre"]]) < 0)      # emission: centre score descending
    # a pool that breaks a condition is refused
    bad = [dict(samples[0]), samples[1], samples[2]]
    bad[0]["scores"] = bad[0]["scores"].copy()
    bad[0]["scores"][1] = bad[0]["scores"][0]
    with pytest.raises(AssertionError):
        br.check_pool_conditions(bad, 100, 0.5)


def test_aleatoric_matrix_is_the_inverse_factor_form():
    rng = np.random.default_rng(1)
    x = rng.normal(0, 0.5, (5, 10))
    sig, bound = br.aleatoric_matrix(x)
    for i in range(5):
        low = np.eye(4)
        low[1, 0], low[2, 0], low[2, 1], low[3, 0], low[3, 1], low[3, 2] = x[i, 8], x[i, 7], x[i, 6], x[i, 3], x[i, 2], x[i, 1]
        d = np.diag(np.exp([x[i, 4], x[i, 9], x[i, 5], x[i, 0]]))
        # Sigma^-1 = L^T D^-1 L
        assert np.allclose(np.linalg.inv(sig[i]), low.T @ np.linalg.inv(d) @ low, rtol=1e-9, atol=1e-12)
    assert (bound > 0).all() and (bound >= br.ALEATORIC_ROUNDINGS * 2.0 ** -24 * 4 * np.abs(sig) * (1 - 1e-12)).all()
    diag, _ = br.aleatoric_matrix(x, use_full_covar=False)
    assert np.array_equal(diag, np.einsum("mi,ij->mij", np.exp(np.stack([x[:, 4], x[:, 9], x[:, 5], x[:, 0]], 1)), np.eye(4)))
    assert not br.aleatoric_matrix(x, has_covar_head=False)[0].any()
    scaled, _ = br.aleatoric_matrix(x, scale=(2.0, 3.0))
    s = np.diag([2.0, 3.0, 2.0, 3.0])
    assert np.allclose(scaled, s @ sig @ s, rtol=1e-12)


def _config(method=None, merge=None, class_uncertainty=False):
    tc = {"bayes_od_config": {"fusion_method": "none"}, "class_uncertainty": class_uncertainty}
    if merge is not None:
        tc["bayes_od_config"]["merge_method"] = merge
    if method is not None:
        tc["uncertainty_method"] = method
    return {"testing_config": tc}


def test_flag_wins_over_yaml_and_the_default_is_bayes_od():
    from bayes_od_rc_amd.run_inference import resolve_uncertainty_method
    assert resolve_uncertainty_method({}) == "bayes_od"
    assert resolve_uncertainty_method(_config()) == "bayes_od"
    assert resolve_uncertainty_method(_config("black_box")) == "black_box"
    assert resolve_uncertainty_method(_config("black_box"), "bayes_od") == "bayes_od"
    assert resolve_uncertainty_method(_config("bayes_od"), "black_box") == "black_box"
    for cfg, flag in ((_config("ensembles"), None), (_config(), "anchor_statistics")):
        with pytest.raises(ValueError, match="uncertainty_method"):
            resolve_uncertainty_method(cfg, flag)


def test_tree_name_is_method_underscore_fusion(tmp_path):
    from bayes_od_rc_amd import writers
    w = writers.PredictionWriter(str(tmp_path), "bdd", 1, "black_box", "none")
    d = writers.PredictionWriter(str(tmp_path), "bdd", 1, "bayes_od", "none")
    base = os.path.join(str(tmp_path), "testing", "bdd", "1")
    assert w.root == os.path.join(base, "black_box_none") and d.root == os.path.join(base, "bayes_od_none")
    assert sorted(os.listdir(w.root)) == ["cat_count", "cat_param", "cov", "data", "mean"]


def test_cli_rejections():
    from bayes_od_rc_amd.run_inference import check_merge_options, check_uncertainty_options
    ns = argparse.Namespace
    assert check_uncertainty_options(_config(), ns()) == ("bayes_od", None)
    assert check_uncertainty_options(_config("black_box"), ns()) == ("black_box", {})
    assert check_uncertainty_options(_config(), ns(uncertainty_method="black_box", bb_min_score=0.25, bb_min_members=3)) == \
        ("black_box", {"min_score": 0.25, "min_members": 3})
    # --merge_terms goes with black box, and still not with the default method
    assert check_merge_options(_config(), ns(uncertainty_method="black_box", merge_terms=True)) == "bayes"
    assert check_merge_options(_config("black_box"), ns(merge_terms=True)) == "bayes"
    with pytest.raises(ValueError, match="merge_terms"):
        check_merge_options(_config("black_box"), ns(uncertainty_method="bayes_od", merge_terms=True))
    bb = dict(uncertainty_method="black_box")
    for kw, word in ((dict(covariance_parts=True), "covariance_parts"), (dict(class_uncertainty=True), "class_uncertainty"),
                     (dict(ensemble=["a.npz", "b.npz"]), "ensemble"), (dict(tta_flip=True), "tta_flip"),
                     (dict(merge_method="mixture"), "merge_method"), (dict(bb_min_members=0), "bb_min_members"),
                     (dict(bb_min_score=-1.0), "bb_min_score")):
        with pytest.raises(ValueError, match=word):
            check_uncertainty_options(_config(), ns(**bb, **kw))
    with pytest.raises(ValueError, match="class_uncertainty"):
        check_uncertainty_options(_config("black_box", class_uncertainty=True), ns())
    with pytest.raises(ValueError, match="merge_method"):
        check_uncertainty_options(_config("black_box", merge="centre"), ns())
    with pytest.raises(ValueError, match="bb_min_score"):
        check_uncertainty_options(_config(), ns(bb_min_score=0.5))
    # the flag brings the default back: everything goes again
    assert check_uncertainty_options(_config("black_box"), ns(uncertainty_method="bayes_od", covariance_parts=True)) == ("bayes_od", None)


def test_cli_parser_rejects_before_building(capsys, tmp_path, monkeypatch):
    monkeypatch.setenv("BAYESOD_DATA_DIR", str(tmp_path))
    from bayes_od_rc_amd import run_inference
    for extra in (["--covariance_parts"], ["--tta_flip"], ["--merge_method", "centre"], ["--class_uncertainty"]):
        with pytest.raises(SystemExit):
            run_inference.main(["--synthetic", "1", "--image_size", "128", "128", "--uncertainty_method", "black_box"] + extra)
        assert "black_box" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        run_inference.main(["--synthetic", "1", "--uncertainty_method", "ensembles"])


def test_pipeline_refuses_before_touching_a_device():
    from bayes_od_rc_amd import inference_utils
    mk = lambda **kw: inference_utils.BayesOdPipeline(None, (128, 128), 1, {}, {}, **kw)
    with pytest.raises(ValueError, match="uncertainty_method"):
        mk(uncertainty_method="blackbox")
    with pytest.raises(ValueError, match="covariance_parts"):
        mk(uncertainty_method="black_box", covariance_parts=True)
    with pytest.raises(ValueError, match="merge_method"):
        mk(uncertainty_method="black_box", merge_method="mixture")
    with pytest.raises(ValueError, match="blackbox_options"):
        mk(blackbox_options={"min_score": 0.5})
    with pytest.raises(ValueError, match="unknown key"):
        mk(uncertainty_method="black_box", blackbox_options={"minimum": 1})


def test_ensemble_and_flip_pipelines_never_see_the_black_box_arguments(monkeypatch):
    """--ensemble / --tta_flip build an EnsemblePipeline, which knows nothing of the uncertainty method: the default method's
    arguments are dropped on the way, a black-box one is refused."""
    from bayes_od_rc_amd import inference_utils, run_inference
    seen = []

    class Model(object):
        mc_dropout_samples = 10
    monkeypatch.setattr(inference_utils, "EnsemblePipeline", lambda *a, **kw: seen.append(kw) or "ensemble")
    monkeypatch.setattr(inference_utils, "BayesOdPipeline", lambda *a, **kw: seen.append(kw) or "single")
    ns = argparse.Namespace
    common = dict(merge_method="bayes", uncertainty_method="bayes_od", blackbox_options=None)
    assert run_inference._make_pipeline(Model(), ns(tta_flip=True), (128, 128), 2, {}, {}, **common) == "ensemble"
    assert run_inference._make_pipeline([Model(), Model()], ns(), (128, 128), 2, {}, {}, **common) == "ensemble"
    assert all("uncertainty_method" not in kw and "blackbox_options" not in kw and kw["merge_method"] == "bayes" for kw in seen)
    del seen[:]
    assert run_inference._make_pipeline(Model(), ns(), (128, 128), 2, {}, {}, merge_method="bayes", uncertainty_method="black_box",
                                        blackbox_options={"min_members": 2}) == "single"
    assert seen[0]["uncertainty_method"] == "black_box" and seen[0]["blackbox_options"] == {"min_members": 2}
    with pytest.raises(ValueError, match="tta_flip"):
        run_inference._make_pipeline(Model(), ns(tta_flip=True), (128, 128), 2, {}, {}, merge_method="bayes",
                                     uncertainty_method="black_box", blackbox_options={})


NEW_SYMBOLS = ("bod_set_uncertainty_method", "bod_get_uncertainty_method", "bod_blackbox_samples", "bod_blackbox_merge",
               "bod_get_sample_detections", "bod_set_sample_detections")


def test_new_symbols_in_the_ctypes_table_and_both_headers():
    from bayes_od_rc_amd import _lib
    header = open(os.path.join(ROOT, "include", "bayesod.h")).read()
    cdef = open(os.path.join(ROOT, "include", "bayesod_cdef.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert "bod_status %s(" % name in header and "bod_status %s(" % name in cdef, name
    assert "enum { BOD_METHOD_BAYES_OD = 0, BOD_METHOD_BLACK_BOX = 1 };" in header
    assert (_lib.BOD_METHOD_BAYES_OD, _lib.BOD_METHOD_BLACK_BOX) == (0, 1)
    assert _lib.UNCERTAINTY_METHODS == {"bayes_od": 0, "black_box": 1}
    import ctypes
    assert ctypes.sizeof(_lib.BodBlackBoxOptions) == 16
    assert [f[0] for f in _lib.BodBlackBoxOptions._fields_] == ["min_score", "min_members", "affinity_threshold", "reserved"]
    assert len(_lib.SIGNATURES["bod_get_sample_detections"][1]) == 8 and len(_lib.SIGNATURES["bod_set_sample_detections"][1]) == 8
