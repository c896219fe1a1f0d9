"""GPU checks of the cluster merge methods (include/bayesod.h, bod_set_merge_method): cluster_merge_kernel fed
IDENTICAL posteriors through bod_set_posterior / bod_set_nms / bod_set_affinity and compared with the float64 restatement in
tests/merge_reference.py under the bounds that file derives entry by entry; the centre method against the posterior rows, bit
for bit; the default method untouched; the option through infer / infer_async / a statistics handle and the CLI.

128 x 128 handles (A = 3 069), mc_samples = 2, no weights unless a test runs the network."""
import os

import numpy as np
import pytest

import merge_reference as mr
from conftest import ANCHOR_CFG, BAYES_CFG, NMS_CFG

pytestmark = pytest.mark.gpu
HW = (128, 128)
KEYS = ("scores", "means", "covs", "counts", "within", "between")


def _anchors():
    from bayes_od_rc_amd.anchor_generator import FpnAnchorGenerator
    return FpnAnchorGenerator(ANCHOR_CFG).generate_all((HW[0], HW[1], 3))


def _engine(c, batch=1, n=2, weights=None, **kw):
    from bayes_od_rc_amd.engine import Engine, make_config
    eng = Engine(make_config(HW, batch=batch, mc_samples=n, num_classes=c, **kw))
    if weights is not None:
        eng.load_weights(weights)
    eng.set_anchors(_anchors())
    return eng


def _inject(eng, img, counts, means, covs, centres):
    eng.set_posterior(img, counts, means, covs, np.zeros(len(counts), np.float32))
    eng._set_centres(img, centres)


def _got(eng, img=0):
    scores, means, covs, counts = eng.get_detections(img)
    within, between, members = eng.get_detection_merge_terms(img)
    return {"scores": scores, "means": means, "covs": covs, "counts": counts, "within": within, "between": between, "members": members}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check_mixture(got, ref, what):
    """Every figure is printed before anything is asserted: the worst error of each array as a fraction of its bound."""
    assert np.array_equal(got["members"], ref["members"]), (what, got["members"], ref["members"])
    worst = {}
    for key in KEYS:
        assert got[key].shape == ref[key].shape, (what, key)
        err = np.abs(got[key].astype(np.float64) - ref[key])
        bound = ref["bound"][key]
        with np.errstate(divide="ignore", invalid="ignore"):
            worst[key] = float(np.nanmax(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0)))) if err.size else 0.0
    print("%s: error / bound " % what + " ".join("%s %.3f" % (k, worst[k]) for k in KEYS))
    for key in KEYS:
        assert worst[key] <= 1.0, (what, key, worst[key])
    assert np.array_equal(got["covs"], got["covs"].transpose(0, 2, 1)) and np.array_equal(got["between"], got["between"].transpose(0, 2, 1))


def _check_centre(got, counts, means, covs, centres, members, what):
    assert np.array_equal(got["members"], members), (what, got["members"], members)
    assert np.array_equal(_bits(got["means"]), _bits(means[centres])), what
    assert np.array_equal(_bits(got["covs"]), _bits(covs[centres])), what
    assert np.array_equal(_bits(got["counts"]), _bits(counts[centres])), what
    assert np.array_equal(_bits(got["within"]), _bits(covs[centres])), what
    assert np.array_equal(_bits(got["between"]), np.zeros((len(centres), 4, 4), np.uint32)), what
    want = np.stack([mr.centre_scores_f32(counts[k]) for k in centres]) if len(centres) else np.zeros_like(got["scores"])
    rel = np.abs(got["scores"].astype(np.float64) - want.astype(np.float64)) / want.astype(np.float64)
    print("%s: centre scores, worst relative error %.3g" % (what, float(rel.max()) if rel.size else 0.0))
    assert rel.size == 0 or rel.max() <= 2.0 ** -23, what


def _cases(c):
    """name -> (counts, means, covs, centres, expected sizes): the shapes of the issue, shared by the mixture and centre tests."""
    out = {}
    for sizes in ((1, 2, 3, 4), (255, 256, 257)):
        rng = np.random.default_rng(10 * c + len(sizes))
        out["sizes_" + "_".join(map(str, sizes))] = mr.clustered_posteriors(rng, sizes, c, singles=5) + (sizes,)
    rng = np.random.default_rng(1500 + c)
    big = mr.clustered_posteriors(rng, (500,), c, singles=1500 - 502)
    assert len(big[0]) == 1500
    out["m1500_cluster_of_500"] = big + ((500,),)
    return out


_CASES = {}


def _case(c, name):
    if c not in _CASES:
        _CASES[c] = _cases(c)
    return _CASES[c][name]


CASE_NAMES = ["sizes_1_2_3_4", "sizes_255_256_257", "m1500_cluster_of_500"]


@pytest.mark.parametrize("c", [4, 8])
@pytest.mark.parametrize("name", CASE_NAMES)
def test_mixture_matches_float64_reference(c, name):
    """Cluster sizes around the `n <= 1` / few-member end and around the block stride of 256 threads and its wrap; M = 1 500 with one
    cluster of 500, where every thread holds two members."""
    counts, means, covs, centres, sizes = _case(c, name)
    ref = mr.merge_reference(counts, means, covs, centres, method="mixture")
    assert tuple(ref["members"]) == tuple(sizes)
    eng = _engine(c)
    eng.set_merge_method("mixture")
    assert eng.merge_method == "mixture"
    _inject(eng, 0, counts, means, covs, centres)
    eng.cluster_fuse()
    _check_mixture(_got(eng), ref, "mixture %s C=%d" % (name, c))
    eng.close()


@pytest.mark.parametrize("c", [4, 8])
@pytest.mark.parametrize("name", CASE_NAMES)
def test_centre_is_the_posterior_row_bit_for_bit(c, name):
    counts, means, covs, centres, sizes = _case(c, name)
    eng = _engine(c)
    eng.set_merge_method("centre")
    _inject(eng, 0, counts, means, covs, centres)
    eng.cluster_fuse()
    assert np.array_equal(eng.get_nms(0), centres)
    _check_centre(_got(eng), counts, means, covs, centres, np.asarray(sizes, np.int32), "centre %s C=%d" % (name, c))
    eng.close()


@pytest.mark.parametrize("c", [4, 8])
@pytest.mark.parametrize("method", ["mixture", "centre"])
def test_hundred_centres_on_the_second_image(c, method):
    """B = 2: K = 100 centres of sizes 1-6 on image 1 (the whole grid row of an image), another M and K on image 0; the batch
    getter pads with zero rows."""
    rng = np.random.default_rng(100 + c)
    sizes1 = tuple(int(s) for s in rng.integers(1, 7, 100))
    imgs = [mr.clustered_posteriors(rng, (5, 3, 9), c, singles=20), mr.clustered_posteriors(rng, sizes1, c, singles=10)]
    assert len(imgs[0][0]) != len(imgs[1][0]) and len(imgs[1][3]) == 100
    eng = _engine(c, batch=2)
    eng.set_merge_method(method)
    for img, x in enumerate(imgs):
        _inject(eng, img, *x)
    eng.cluster_fuse()
    batch = eng.get_detection_merge_terms_batch()
    for img, (counts, means, covs, centres) in enumerate(imgs):
        ref = mr.merge_reference(counts, means, covs, centres, method=method)
        if img == 1:
            assert tuple(ref["members"]) == sizes1
        got = _got(eng, img)
        if method == "mixture":
            _check_mixture(got, ref, "mixture image %d C=%d" % (img, c))
        else:
            _check_centre(got, counts, means, covs, centres, ref["members"], "centre image %d C=%d" % (img, c))
        k = len(centres)
        for key in ("within", "between", "members"):
            assert np.array_equal(batch[key][img, :k], got[key]) and not batch[key][img, k:].any(), key
    eng.close()


@pytest.mark.parametrize("c", [4, 8])
def test_mixture_of_single_member_clusters_equals_centre(c):
    rng = np.random.default_rng(31 + c)
    counts, means, covs, centres = mr.clustered_posteriors(rng, (1, 1, 1, 1, 1, 1), c, singles=7, distractors=2)
    eng = _engine(c)
    got = {}
    for method in ("centre", "mixture"):
        eng.set_merge_method(method)
        _inject(eng, 0, counts, means, covs, centres)
        eng.cluster_fuse()
        got[method] = _got(eng)
    assert tuple(got["mixture"]["members"]) == (1,) * 6
    for key in ("means", "covs", "within", "between", "members"):
        assert np.array_equal(_bits(got["mixture"][key]) if key != "members" else got["mixture"][key],
                              _bits(got["centre"][key]) if key != "members" else got["centre"][key]), key
    eng.close()


@pytest.mark.parametrize("c", [4, 8])
@pytest.mark.parametrize("method", ["mixture", "centre"])
def test_callers_affinity_columns(c, method):
    """bod_set_affinity: one column excludes every row (members = 0: the centre's row), one excludes the centre itself but keeps
    the others, one is the IoU; the columns are one-shot."""
    rng = np.random.default_rng(77 + c)
    counts, means, covs, centres = mr.clustered_posteriors(rng, (4, 6, 5), c, singles=6)
    m = len(counts)
    iou = mr.iou_affinity(means)
    affinity = np.zeros((m, m))
    affinity[:, centres] = iou[:, centres]
    affinity[:, centres[0]] = 0.0                                   # nobody
    affinity[centres[1], centres[1]] = 0.0                          # everybody but the centre
    ref = mr.merge_reference(counts, means, covs, centres, affinity=affinity, method=method)
    assert tuple(ref["members"]) == (0, 5, 5)
    eng = _engine(c)
    eng.set_merge_method(method)
    _inject(eng, 0, counts, means, covs, centres)
    eng.set_affinity(0, np.ascontiguousarray(affinity[:, centres].T, np.float32))
    eng.cluster_fuse()
    got = _got(eng)
    if method == "mixture":
        _check_mixture(got, ref, "mixture, caller's affinity C=%d" % c)
        assert not np.array_equal(got["means"][1], means[centres[1]])          # the centre is not among its own members
    else:
        _check_centre(got, counts, means, covs, centres, ref["members"], "centre, caller's affinity C=%d" % c)
    # members = 0: the centre's own row, bit for bit, under either method
    assert np.array_equal(_bits(got["means"][0]), _bits(means[centres[0]])) and np.array_equal(_bits(got["covs"][0]), _bits(covs[centres[0]]))
    assert np.array_equal(_bits(got["counts"][0]), _bits(counts[centres[0]])) and not got["between"][0].any()
    # one-shot: the next cluster stage is back on the IoU
    eng.cluster_fuse()
    assert tuple(_got(eng)["members"]) == (4, 6, 5)
    eng.close()


@pytest.mark.parametrize("c", [4, 8])
def test_default_method_is_untouched_after_a_mixture(c):
    """A handle that ran mixture and was set back to bayes gives the detections of a fresh handle, bit for bit, and has no terms."""
    rng = np.random.default_rng(55 + c)
    counts, means, covs, centres = mr.clustered_posteriors(rng, (1, 2, 3, 4, 7, 40), c, singles=5)
    used, fresh = _engine(c), _engine(c)
    assert used.merge_method == "bayes" and fresh.merge_method == "bayes"
    used.set_merge_method("mixture")
    _inject(used, 0, counts, means, covs, centres)
    used.cluster_fuse()
    mixture = used.get_detections(0)
    used.get_detection_merge_terms(0)
    used.set_merge_method("bayes")
    assert used.merge_method == "bayes"
    dets = []
    for eng in (used, fresh):
        _inject(eng, 0, counts, means, covs, centres)
        eng.cluster_fuse()
        dets.append(eng.get_detections(0))
    for a, b in zip(*dets):
        assert a.shape[0] == len(centres) and np.array_equal(_bits(a), _bits(b))
    assert not np.array_equal(mixture[2], dets[0][2])                          # (the factor 70 alone tells them apart)
    for eng in (used, fresh):
        with pytest.raises(ValueError, match="BOD_MERGE_BAYES"):
            eng.get_detection_merge_terms(0)
        with pytest.raises(ValueError, match="BOD_MERGE_BAYES"):
            eng.get_detection_merge_terms_batch()
    with pytest.raises(ValueError, match="unknown method"):
        used._chk(used.lib.bod_set_merge_method(used.h, 3))
    assert used.merge_method == "bayes"
    used.close()
    fresh.close()


# ---- end to end with synthetic weights ---------------------------------------------------------------------------------------------
def _weights(c):
    from bayes_od_rc_amd import synthetic
    return synthetic.make_weights(c, 9, cls_fg_bias=-1.0)


def _frames(batch, seed):
    from bayes_od_rc_amd import synthetic
    return synthetic.make_frames(batch, HW[0], HW[1], seed=seed)


def _centre_equals_posterior_rows(eng, what):
    total = 0
    for img in range(eng.B):
        post, idx = eng.get_posterior(img), eng.get_nms(img)
        got = _got(eng, img)
        assert got["means"].shape[0] == len(idx)
        thr = float(eng.cfg.nms_iou_threshold)
        members = mr.member_columns(post["means"], idx, thr=thr, guard=1e-6).sum(axis=0).astype(np.int32)
        _check_centre(got, post["counts"], post["means"], post["covs"], idx, members, "%s image %d" % (what, img))
        total += len(idx)
    assert total > 0, "no detections: the test shows nothing"


@pytest.mark.parametrize("c", [4, 8])
def test_infer_under_centre_reports_the_posterior_rows(c):
    eng = _engine(c, batch=2, n=4, weights=_weights(c), bayes_od_config=BAYES_CFG, nms_config=NMS_CFG)
    eng.set_merge_method("centre")
    eng.infer(_frames(2, 1), seed=2024, first_image_id=0)
    _centre_equals_posterior_rows(eng, "infer, centre C=%d" % c)
    eng.close()


@pytest.mark.parametrize("c", [4, 8])
def test_async_tickets_carry_the_mixture_and_its_terms(c):
    """B = 2, two batches in flight: collect + get_detection_merge_terms_batch(slot) equal the synchronous results bit for bit."""
    eng = _engine(c, batch=2, n=4, weights=_weights(c), bayes_od_config=BAYES_CFG, nms_config=NMS_CFG)
    eng.set_merge_method("mixture")
    batches = [_frames(2, s) for s in (31, 99)]
    want = []
    for i, frames in enumerate(batches):
        eng.infer(frames, seed=77 + i, first_image_id=5 + 10 * i)
        want.append((eng.get_detections_batch(), eng.get_detection_merge_terms_batch()))
    assert want[0][0]["num"].sum() > 0 and want[1][0]["num"].sum() > 0
    assert not np.array_equal(want[0][1]["within"], want[1][1]["within"])
    slots = [eng.infer_async(frames, seed=77 + i, first_image_id=5 + 10 * i) for i, frames in enumerate(batches)]
    assert sorted(slots) == [0, 1]
    for slot, (det, terms) in zip(slots, want):
        got = eng.collect(slot)
        got_terms = eng.get_detection_merge_terms_batch(slot)
        assert np.array_equal(got["num"], det["num"])
        for img, n in enumerate(det["num"]):
            for key in ("scores", "means", "covs", "counts"):
                assert np.array_equal(_bits(got[key][img, :n]), _bits(det[key][img, :n])), key
            for key in ("within", "between"):
                assert np.array_equal(_bits(got_terms[key][img]), _bits(terms[key][img])), key
            assert np.array_equal(got_terms["members"][img], terms["members"][img]) and (terms["members"][img, :n] >= 1).all()
            cov = terms["within"][img, :n] + terms["between"][img, :n]
            assert np.array_equal(_bits(cov), _bits(det["covs"][img, :n]))
    ptrs = eng.device_detection_merge_terms_pointers(slots[1])
    assert all(p != 0 for p, _ in ptrs.values()) and ptrs["members"][1] == (2, eng.K)
    eng.close()


@pytest.mark.parametrize("c", [4, 8])
def test_statistics_handle_honours_the_method(c):
    """stat_forward x 2 -> stat_posterior -> nms -> cluster_fuse under centre, then under mixture on the same posterior."""
    eng = _engine(c, batch=1, n=2, weights=_weights(c), bayes_od_config=BAYES_CFG, nms_config=NMS_CFG, mc_statistics=True,
                  mc_ensemble_size=4)
    frames = _frames(1, 7)
    eng.set_merge_method("centre")
    for base in (0, 2):
        eng.stat_forward(frames, seed=11, first_image_id=3, sample_base=base)
    eng.stat_posterior(seed=11, first_image_id=3)
    eng.nms()
    eng.cluster_fuse()
    _centre_equals_posterior_rows(eng, "statistics handle, centre C=%d" % c)
    post, idx = eng.get_posterior(0), eng.get_nms(0)
    eng.set_merge_method("mixture")
    eng.cluster_fuse()
    ref = mr.merge_reference(post["counts"], post["means"], post["covs"], idx, thr=float(eng.cfg.nms_iou_threshold), method="mixture", guard=1e-6)
    _check_mixture(_got(eng), ref, "statistics handle, mixture C=%d" % c)
    eng.close()


def test_refusals_carry_the_reason_and_leave_the_handle_working():
    from bayes_od_rc_amd.engine import Engine, make_config
    rng = np.random.default_rng(3)
    counts, means, covs, centres = mr.clustered_posteriors(rng, (3, 2), 8, singles=3)
    for kw in (dict(covariance_parts=True), dict(class_parts=True)):
        eng = _engine(8, **kw)
        for method in ("centre", "mixture"):
            with pytest.raises(ValueError, match="covariance_parts.*Bayesian fuse"):
                eng.set_merge_method(method)
        assert eng.merge_method == "bayes"
        eng.set_merge_method("bayes")                                # the default is no refusal
        _inject(eng, 0, counts, means, covs, centres)
        eng.cluster_fuse()
        assert eng.get_detections(0)[1].shape == (2, 4)
        eng.close()
    train = Engine(make_config(HW, batch=1, mc_samples=1, training=True))
    for method in ("bayes", "mixture"):
        with pytest.raises(ValueError, match="training handle"):
            train.set_merge_method(method)
    assert train.merge_method == "bayes"
    train.synchronize()
    train.close()


def test_clustering_entry_point_sets_the_method_on_every_call():
    """inference_utils.bayes_od_clustering shares its stand-alone handle between calls: mixture, then the default, then centre."""
    from bayes_od_rc_amd import inference_utils
    rng = np.random.default_rng(9)
    counts, means, covs, centres = mr.clustered_posteriors(rng, (3, 5, 1), 8, singles=3)
    ref = mr.merge_reference(counts, means, covs, centres, method="mixture")
    out = inference_utils.bayes_od_clustering(counts, means, covs, centres, affinity_threshold=0.5, merge_method="mixture",
                                              return_merge_terms=True)
    assert len(out) == 7 and out[1].shape == (3, 4, 1)
    got = dict(zip(("scores", "means", "covs", "counts", "within", "between", "members"), out))
    got["means"] = got["means"][:, :, 0]
    _check_mixture(got, ref, "bayes_od_clustering, mixture")
    default = inference_utils.bayes_od_clustering(counts, means, covs, centres, affinity_threshold=0.5)
    assert len(default) == 4 and not np.array_equal(default[2], out[2])
    explicit = inference_utils.bayes_od_clustering(counts, means, covs, centres, affinity_threshold=0.5, merge_method="bayes")
    for a, b in zip(default, explicit):
        assert np.array_equal(_bits(a), _bits(b))
    centre = inference_utils.bayes_od_clustering(counts, means, covs, centres, affinity_threshold=0.5, merge_method="centre")
    assert np.array_equal(_bits(centre[2]), _bits(covs[centres]))


def test_run_inference_cli_writes_the_mixture_tree_beside_the_default(tmp_path, monkeypatch):
    monkeypatch.setenv("BAYESOD_DATA_DIR", str(tmp_path))
    from bayes_od_rc_amd import run_inference
    common = ["--gpu_device", "0", "--data_split", "test", "--synthetic", "2", "--image_size", "128", "128"]
    root = run_inference.main(common + ["--merge_method", "mixture", "--merge_terms"])
    assert root.endswith(os.path.join("predictions", "testing", "bdd", "101", "bayes_od_none-mixture"))
    for i in range(2):
        k = np.load(os.path.join(root, "mean", "%06d.npy" % i)).shape[0]
        cov = np.load(os.path.join(root, "cov", "%06d.npy" % i))
        within = np.load(os.path.join(root, "merge_within", "%06d.npy" % i))
        between = np.load(os.path.join(root, "merge_between", "%06d.npy" % i))
        members = np.load(os.path.join(root, "merge_members", "%06d.npy" % i))
        assert within.shape == (k, 4, 4) and between.shape == (k, 4, 4) and members.shape == (k,) and members.dtype == np.int32
        assert np.array_equal(within + between, cov) and (members >= 1).all()
    default = run_inference.main(common)
    assert default.endswith(os.path.join("predictions", "testing", "bdd", "101", "bayes_od_none"))
    assert sorted(os.listdir(default)) == ["cat_count", "cat_param", "cov", "data", "mean"]
    with pytest.raises(SystemExit):
        run_inference.main(common + ["--merge_method", "centre", "--covariance_parts"])
