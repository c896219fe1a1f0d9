"""GPU checks of black-box MC dropout (include/bayesod.h, bod_set_uncertainty_method): stage 1 against
bod_validation_post + bod_nms of a second handle that holds the sample in position 0, bit for bit; the sample covariances against
float64; stage 2 on injected sample detections against tests/blackbox_reference.py under the bounds that file derives; the method
through infer / infer_async and the CLI; the refusals.

128 x 128 handles (A = 3 069) unless a test says otherwise; no weights unless a test runs the network."""
import os

import numpy as np
import pytest

import blackbox_reference as br
import post_reference
from conftest import ANCHOR_CFG

pytestmark = pytest.mark.gpu
HW = (128, 128)
KEYS = ("scores", "means", "covs", "counts", "within", "between")


def _anchors(hw=HW):
    from bayes_od_rc_amd.anchor_generator import FpnAnchorGenerator
    return FpnAnchorGenerator(ANCHOR_CFG).generate_all((hw[0], hw[1], 3))


def _engine(c, batch=2, n=3, hw=HW, kmax=100, weights=None, **kw):
    from bayes_od_rc_amd.engine import Engine, make_config
    nms = {"max_output_size": kmax, "iou_threshold": 0.5, "soft_nms_sigma": 0.5}
    eng = Engine(make_config(hw, batch=batch, mc_samples=n, num_classes=c, nms_config=nms, **kw))
    if weights is not None:
        eng.load_weights(weights)
    eng.set_anchors(_anchors(hw))
    return eng


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _raw(c, hw=HW, b=2, n=3, seed=0):
    a = _anchors(hw).shape[0]
    return post_reference.random_raw(np.random.default_rng(seed), b, n, a, c=c)


def _validation_rows(ref, raw, n):
    """The reference route for sample n of every image: the sample in position 0 of a second handle, validation_post, nms."""
    ref.set_raw(*[np.ascontiguousarray(np.roll(t, -n, axis=1)) for t in raw])
    ref.validation_post()
    ref.nms()
    out = []
    for b in range(ref.B):
        post, sel = ref.get_posterior(b), ref.get_nms(b)
        out.append({"anchor_index": post["anchor_index"][sel], "scores": post["score"][sel], "means": post["means"][sel],
                    "kept": len(post["ranking"])})
    return out


def _assert_same_rows(got, want, what):
    assert np.array_equal(got["anchor_index"], want["anchor_index"]), what
    assert np.array_equal(_bits(got["scores"]), _bits(want["scores"])), what
    assert np.array_equal(_bits(got["means"]), _bits(want["means"])), what


# ---- 1. the per-sample stage against the existing stages, bit for bit -------------------------------------------------------
@pytest.mark.parametrize("c", [4, 8])
def test_sample_stage_equals_validation_post_and_nms(c):
    raw = list(_raw(c, seed=c))
    raw[0][0, 1, :, -1] += 100.0                            # (image 0, sample 1): every anchor background
    eng, ref = _engine(c), _engine(c)
    eng.set_uncertainty_method("black_box")
    assert eng.uncertainty_method == "black_box"
    eng.set_raw(*raw)
    eng.blackbox_samples()
    total = 0
    for n in range(3):
        want = _validation_rows(ref, raw, n)
        for b in range(2):
            got = eng.get_sample_detections(b, n)
            _assert_same_rows(got, want[b], "C=%d image %d sample %d" % (c, b, n))
            total += len(got["anchor_index"])
            if (b, n) == (0, 1):
                assert want[b]["kept"] == 0 and len(got["anchor_index"]) == 0
    assert total > 100
    eng.close(); ref.close()


def test_sample_stage_beyond_the_nms_lds_capacity():
    """256 x 256 (A = 12 276): more than 6 144 candidates on (image 1, sample 2) and on (image 0, sample 1), where nms_kernel keeps
    its queue in the work buffers -- indexed by the virtual image, not the image."""
    hw, c = (256, 256), 8
    raw = list(_raw(c, hw=hw, seed=5))
    raw[0][1, 2, :, -1] -= 12.0
    raw[0][0, 1, :, -1] -= 12.0
    eng, ref = _engine(c, hw=hw), _engine(c, hw=hw)
    eng.set_uncertainty_method("black_box")
    eng.set_raw(*raw)
    eng.blackbox_samples()
    for n in range(3):
        want = _validation_rows(ref, raw, n)
        if n == 2:
            assert want[1]["kept"] > 6144
        if n == 1:
            assert want[0]["kept"] > 6144
        for b in range(2):
            _assert_same_rows(eng.get_sample_detections(b, n), want[b], "256x256 image %d sample %d" % (b, n))
    eng.close(); ref.close()


# ---- 2. the sample covariances against float64 --------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(use_full_covar=True), dict(use_full_covar=False), dict(has_covar_head=False),
                                dict(use_full_covar=True, dataset_name="kitti", orig_size=(192, 320))],
                         ids=["full", "diagonal", "no_head", "kitti"])
def test_sample_covariances_against_float64(kw):
    c = 8
    raw = _raw(c, seed=11)
    eng = _engine(c, **kw)
    eng.set_uncertainty_method("black_box")
    head = kw.get("has_covar_head", True)
    eng.set_raw(raw[0], raw[1], raw[2] if head else None)
    eng.blackbox_samples()
    scale = (192 / 128.0, 320 / 128.0) if "dataset_name" in kw else None
    plain = None
    if scale:                                               # the means of an unscaled handle, times S in float32: one multiplication
        plain = _engine(c)
        plain.set_uncertainty_method("black_box")
        plain.set_raw(*raw)
        plain.blackbox_samples()
    worst, rows = 0.0, 0
    for b in range(2):
        for n in range(3):
            got = eng.get_sample_detections(b, n)
            ref, bound = br.aleatoric_matrix(raw[2][b, n, got["anchor_index"]], kw.get("use_full_covar", True), head, scale)
            err = np.abs(got["covs"].astype(np.float64) - ref)
            if not head:
                assert not got["covs"].any()
            else:
                with np.errstate(divide="ignore", invalid="ignore"):     # (a zero bound -- the diagonal form's off-diagonal -- allows no error)
                    ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
                worst = max(worst, float(ratio.max()) if ratio.size else 0.0)
            rows += len(err)
            if scale:
                base = plain.get_sample_detections(b, n)
                assert np.array_equal(got["anchor_index"], base["anchor_index"])
                s = np.array([scale[0], scale[1], scale[0], scale[1]], np.float32)
                assert np.array_equal(_bits(got["means"]), _bits(base["means"] * s))
    print("sample covariances %s: %d rows, worst error / bound %.3f" % (kw, rows, worst))
    assert rows > 100 and worst <= 1.0
    eng.close()
    if plain:
        plain.close()


# ---- 3. min_score ------------------------------------------------------------------------------------------------------------
def test_min_score_keeps_exactly_the_rows_at_or_above_it():
    c = 8
    raw = _raw(c, seed=3)
    eng = _engine(c)
    eng.set_uncertainty_method("black_box")
    eng.set_raw(*raw)
    eng.blackbox_samples()
    full = [[eng.get_sample_detections(b, n) for n in range(3)] for b in range(2)]
    eng.set_uncertainty_method("black_box", min_score=0.9)
    eng.blackbox_samples()
    dropped = 0
    for b in range(2):
        for n in range(3):
            keep = ~(full[b][n]["scores"].max(axis=1) < np.float32(0.9))
            got = eng.get_sample_detections(b, n)
            for key in ("anchor_index", "scores", "means", "covs"):
                assert np.array_equal(got[key], full[b][n][key][keep]), (b, n, key)
            dropped += int((~keep).sum())
    assert dropped > 10
    eng.close()


# ---- 4. the pool merge on injected sample detections ----------------------------------------------------------------------------
def _spread(size, n_samples=3):
    """`size` members dealt round-robin to the samples."""
    return [i % n_samples for i in range(size)]


POOLS = {
    # sizes 1, 2, 3; one member from each sample; two members from the same sample
    "small": [[0], [1], [2], [0, 1], [1, 2], [0, 1, 2], [1, 1], [2, 2, 0], [0, 0, 0]],
    "c255": [_spread(255)] + [[n] for n in (0, 1, 2, 0, 1, 2)],
    "c256": [_spread(256)] + [[n] for n in (0, 1, 2, 0, 1, 2)],
    "c257": [_spread(257)] + [[n] for n in (0, 1, 2, 0, 1, 2)],
    "many": [[i % 3] for i in range(130)] + [[0, 1], [1, 2, 0]],          # more than Kmax = 100 clusters
}
_POOL_CACHE = {}


def _pool(name, c):
    if (name, c) not in _POOL_CACHE:
        rng = np.random.default_rng(1000 * c + sorted(POOLS).index(name))
        _POOL_CACHE[(name, c)] = br.clustered_pool(rng, POOLS[name], c, 3, 100)
    return _POOL_CACHE[(name, c)]


def _inject(eng, img, samples):
    for n, s in enumerate(samples):
        eng.set_sample_detections(img, n, s["scores"], s["means"], s["covs"], s.get("anchor_index"))


def _empty(c, n_samples):
    return [{"scores": np.zeros((0, c), np.float32), "means": np.zeros((0, 4), np.float32), "covs": np.zeros((0, 4, 4), np.float32)}
            for _ in range(n_samples)]


def _got(eng, img):
    scores, means, covs, counts = eng.get_detections(img)
    within, between, members = eng.get_detection_merge_terms(img)
    return {"scores": scores, "means": means, "covs": covs, "counts": counts, "within": within, "between": between, "members": members}


def _check(got, ref, what):
    """Every figure is printed before anything is asserted: the worst error of each array as a fraction of its bound."""
    assert np.array_equal(got["members"], ref["members"]), (what, got["members"], ref["members"])
    worst = {}
    for key in KEYS:
        assert got[key].shape == ref[key].shape, (what, key, got[key].shape, ref[key].shape)
        err = np.abs(got[key].astype(np.float64) - ref[key])
        bound = ref["bound"][key]
        with np.errstate(divide="ignore", invalid="ignore"):
            worst[key] = float(np.nanmax(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0)))) if err.size else 0.0
    print("%s: error / bound " % what + " ".join("%s %.3f" % (k, worst[k]) for k in KEYS))
    for key in KEYS:
        assert worst[key] <= 1.0, (what, key, worst[key])


@pytest.mark.parametrize("min_members", [1, 3])
@pytest.mark.parametrize("c", [4, 8])
@pytest.mark.parametrize("name", sorted(POOLS))
def test_pool_merge_matches_float64_reference(name, c, min_members):
    """Image 1 of B = 2 holds the pool, image 0 an empty one."""
    samples = _pool(name, c)
    ref = br.pool_merge_reference(samples, 100, 0.5, min_members)
    if name == "many":
        assert len(ref["members"]) == (100 if min_members == 1 else 1)
    eng = _engine(c)
    eng.set_uncertainty_method("black_box", min_members=min_members)
    _inject(eng, 0, _empty(c, 3))
    _inject(eng, 1, samples)
    eng.blackbox_merge()
    assert eng.get_detections(0)[0].shape[0] == 0
    _check(_got(eng, 1), ref, "pool %s C=%d min_members=%d" % (name, c, min_members))
    eng.close()


def test_pool_merge_two_images_with_different_pools_and_threshold():
    c = 8
    p0, p1 = _pool("small", c), _pool("c257", c)
    eng = _engine(c)
    eng.set_uncertainty_method("black_box", affinity_threshold=0.7)
    _inject(eng, 0, p0)
    _inject(eng, 1, p1)
    eng.blackbox_merge()
    br.check_pool_conditions(p0, 100, 0.7); br.check_pool_conditions(p1, 100, 0.7)
    _check(_got(eng, 0), br.pool_merge_reference(p0, 100, 0.7), "two images, image 0")
    _check(_got(eng, 1), br.pool_merge_reference(p1, 100, 0.7), "two images, image 1")
    eng.close()


def test_pool_merge_beyond_the_lds_capacity():
    """N = 30, Kmax = 512: a pool of 15 360 entries, which lives in the global work buffers.  620 of them are filled, the last
    ranks of the last sample included."""
    c, n_s, kmax = 8, 30, 512
    rng = np.random.default_rng(77)
    clusters = [[int(s) for s in rng.integers(0, n_s, size)] for size in (1, 2, 3, 40, 64, 65)] + [[29] * 3] + \
               [[int(rng.integers(0, n_s))] for _ in range(442)]
    samples = br.clustered_pool(rng, clusters, c, n_s, kmax)
    ref = br.pool_merge_reference(samples, kmax)
    eng = _engine(c, batch=1, n=n_s, kmax=kmax)
    eng.set_uncertainty_method("black_box")
    _inject(eng, 0, samples)
    eng.blackbox_merge()
    _check(_got(eng, 0), ref, "pool of 15 360")
    eng.close()


# ---- 5. a single-member cluster ------------------------------------------------------------------------------------------------
def test_single_member_cluster_is_its_sample_detection_byte_for_byte():
    c = 8
    samples = _pool("small", c)
    ref = br.pool_merge_reference(samples, 100)
    eng = _engine(c)
    eng.set_uncertainty_method("black_box")
    _inject(eng, 0, samples)
    _inject(eng, 1, _empty(c, 3))
    eng.blackbox_merge()
    got = _got(eng, 0)
    singles = np.nonzero(ref["members"] == 1)[0]
    assert len(singles) == 3
    for k in singles:
        n, rank = divmod(int(ref["centre"][k]), 100)
        s = samples[n]
        assert np.array_equal(_bits(got["means"][k]), _bits(s["means"][rank]))
        assert np.array_equal(_bits(got["covs"][k]), _bits(s["covs"][rank])) and np.array_equal(_bits(got["within"][k]), _bits(s["covs"][rank]))
        assert np.array_equal(_bits(got["scores"][k]), _bits(s["scores"][rank])) and np.array_equal(_bits(got["counts"][k]), _bits(s["scores"][rank]))
        assert not _bits(got["between"][k]).any()
    eng.close()


# ---- 6. with synthetic weights ---------------------------------------------------------------------------------------------------
def _weights():
    from bayes_od_rc_amd import synthetic
    return synthetic.make_weights(cls_fg_bias=-1.0)


def _frames(b=2):
    from bayes_od_rc_amd import synthetic
    return synthetic.make_frames(b, HW[0], HW[1], seed=1)


def _valid_rows_equal(a, b):
    assert np.array_equal(a["num"], b["num"])
    for key in ("scores", "means", "covs", "counts"):
        for i, k in enumerate(a["num"]):
            assert np.array_equal(_bits(a[key][i, :k]), _bits(b[key][i, :k])), (key, i)


def test_infer_equals_the_stages_and_the_pipelined_form_and_switching_back_is_clean():
    w, frames = _weights(), _frames()
    eng = _engine(8, n=3, weights=w)
    never = _engine(8, n=3, weights=w)
    never.infer(frames, seed=5)
    want_default = never.get_detections_batch()
    bytes_before = eng.device_bytes
    assert bytes_before == never.device_bytes               # nothing of the method exists before the first switch
    eng.set_uncertainty_method("black_box")
    assert eng.device_bytes > bytes_before
    eng.infer(frames, seed=5)
    a = eng.get_detections_batch()
    terms_a = eng.get_detection_merge_terms_batch()
    assert a["num"].min() > 0
    eng.forward(frames, seed=5)
    eng.blackbox_samples()
    eng.blackbox_merge()
    _valid_rows_equal(a, eng.get_detections_batch())
    terms_b = eng.get_detection_merge_terms_batch()
    for key in ("within", "between", "members"):
        assert np.array_equal(terms_a[key], terms_b[key]), key
    for i, k in enumerate(a["num"]):
        assert np.array_equal(a["covs"][i, :k], terms_a["within"][i, :k] + terms_a["between"][i, :k])
        assert (terms_a["members"][i, :k] >= 1).all() and terms_a["members"][i, :k].max() <= 3 * 100
    slot = eng.infer_async(frames, seed=5)
    _valid_rows_equal(a, eng.collect(slot))
    eng.set_uncertainty_method("bayes_od")
    eng.infer(frames, seed=5)
    _valid_rows_equal(want_default, eng.get_detections_batch())
    eng.close(); never.close()


# ---- 7. N = 1 -------------------------------------------------------------------------------------------------------------------
def test_single_sample_handle_gives_the_validation_detections():
    """mc_samples = 1: the pool is the one sample's NMS rows.  Soft-NMS survivors may still exceed the threshold with each other
    under the reference's +1 formula (small boxes: a (w+1)(h+1) intersection over (w-1)(h-1) areas), so the rows stay alone --
    members = 1, the detections are the validation detections -- when theta lies above their largest pairwise affinity; the test
    reads that affinity off the validation rows and sets theta 0.05 above it.  At the default theta every row is still consumed
    exactly once."""
    w, frames = _weights(), _frames()
    eng = _engine(8, n=1, weights=w)
    with pytest.raises(ValueError, match="mc_samples >= 2"):
        eng.infer(frames, seed=5)
    eng.forward(frames, seed=5)
    eng.validation_post()
    eng.nms()
    rows, theta = [], 0.5
    for b in range(2):
        post, sel = eng.get_posterior(b), eng.get_nms(b)
        assert len(sel) > 1
        aff = post_reference.iou_plus1(br.corners_f32(post["means"][sel]))
        theta = max(theta, float(aff[~np.eye(len(sel), dtype=bool)].max()) + 0.05)
        rows.append({"means": post["means"][sel], "scores": post["score"][sel]})
    eng.set_uncertainty_method("black_box")
    eng.infer(frames, seed=5)
    for b in range(2):
        members = _got(eng, b)["members"]
        print("N = 1, default theta, image %d: %d validation rows, cluster sizes %s" % (b, len(rows[b]["means"]), np.bincount(members)))
        assert members.sum() == len(rows[b]["means"]) and (members >= 1).all()
    eng.set_uncertainty_method("black_box", affinity_threshold=theta)
    eng.infer(frames, seed=5)
    for b in range(2):
        got, want = _got(eng, b), rows[b]
        top = want["scores"].max(axis=1)
        order = np.lexsort((np.arange(len(top)), -top))     # emission order: top score descending, ties to the lower rank
        assert np.array_equal(got["members"], np.ones(len(top), np.int32))
        assert np.array_equal(_bits(got["means"]), _bits(want["means"][order]))
        assert np.array_equal(_bits(got["scores"]), _bits(want["scores"][order]))
        assert np.array_equal(_bits(got["counts"]), _bits(want["scores"][order]))
        assert np.array_equal(_bits(got["covs"]), _bits(got["within"])) and not _bits(got["between"]).any()
    eng.close()


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_are_invalid_arg_with_their_reason():
    from bayes_od_rc_amd import _lib
    import ctypes as C

    def status(eng, method, opt=None):
        st = eng.lib.bod_set_uncertainty_method(eng.h, method, None if opt is None else C.byref(opt))
        return st, eng.lib.bod_last_error(eng.h).decode()

    plain = _engine(8)
    st, msg = status(plain, 7)
    assert st == _lib.BOD_ERR_INVALID_ARG and "unknown method" in msg
    for opt, word in ((_lib.BodBlackBoxOptions(0.0, 0, 0.0, 0), "min_members"), (_lib.BodBlackBoxOptions(-1.0, 1, 0.0, 0), "min_score"),
                      (_lib.BodBlackBoxOptions(0.0, 1, float("nan"), 0), "affinity_threshold"), (_lib.BodBlackBoxOptions(0.0, 1, 0.0, 3), "reserved")):
        st, msg = status(plain, 1, opt)
        assert st == _lib.BOD_ERR_INVALID_ARG and word in msg, msg
    assert plain.uncertainty_method == "bayes_od"
    # stage entries before the first switch
    with pytest.raises(ValueError, match="bod_set_uncertainty_method"):
        plain.blackbox_merge()
    plain.set_merge_method("mixture")
    st, msg = status(plain, 1)
    assert st == _lib.BOD_ERR_INVALID_ARG and "merge method" in msg
    plain.set_merge_method("bayes")
    assert status(plain, 1, None)[0] == _lib.BOD_OK          # NULL options: {0, 1, 0}
    assert plain.uncertainty_method == "black_box"
    with pytest.raises(ValueError, match="BOD_METHOD_BLACK_BOX"):
        plain.set_merge_method("centre")
    plain.set_merge_method("bayes")
    with pytest.raises(ValueError, match="has not run"):
        plain.blackbox_merge()
    plain.close()
    for kw, word in ((dict(mc_statistics=True), "statistics handle"), (dict(covariance_parts=True), "covariance_parts"),
                     (dict(class_parts=True), "covariance_parts")):
        eng = _engine(8, **kw)
        st, msg = status(eng, 1)
        assert st == _lib.BOD_ERR_INVALID_ARG and word in msg, msg
        assert eng.uncertainty_method == "bayes_od"
        eng.close()
    from bayes_od_rc_amd.engine import Engine, make_config
    tr = Engine(make_config(HW, batch=1, mc_samples=1, training=True))
    st, msg = status(tr, 1)
    assert st == _lib.BOD_ERR_INVALID_ARG and "training handle" in msg
    tr.close()


# ---- 9. the CLI -----------------------------------------------------------------------------------------------------------------
def test_run_inference_cli_writes_the_black_box_tree(tmp_path, monkeypatch):
    monkeypatch.setenv("BAYESOD_DATA_DIR", str(tmp_path))
    from bayes_od_rc_amd import offline_eval, run_inference
    root = run_inference.main(["--gpu_device", "0", "--data_split", "test", "--synthetic", "2", "--image_size", "128", "128",
                               "--uncertainty_method", "black_box", "--merge_terms"])
    assert root.endswith(os.path.join("predictions", "testing", "bdd", "101", "black_box_none"))
    assert sorted(os.listdir(root)) == ["cat_count", "cat_param", "cov", "data", "mean", "merge_between", "merge_members", "merge_within"]
    frames = ["%06d" % i for i in range(2)]
    for f in frames:
        k = np.load(os.path.join(root, "mean", f + ".npy")).shape[0]
        cov = np.load(os.path.join(root, "cov", f + ".npy"))
        within, between = (np.load(os.path.join(root, d, f + ".npy")) for d in ("merge_within", "merge_between"))
        members = np.load(os.path.join(root, "merge_members", f + ".npy"))
        assert np.load(os.path.join(root, "cat_param", f + ".npy")).shape[0] == k
        assert np.load(os.path.join(root, "cat_count", f + ".npy")).shape[0] == k
        assert within.shape == (k, 4, 4) and between.shape == (k, 4, 4) and members.shape == (k,) and members.dtype == np.int32
        assert np.array_equal(within + between, cov) and (members >= 1).all()
    records = offline_eval.entropy_ranked_predictions(root, frames)
    assert len(records) == sum(np.load(os.path.join(root, "mean", f + ".npy")).shape[0] for f in frames) and len(records) > 0
    assert all(np.isfinite(r["entropy_score"]) for r in records)
