"""GPU parity of the loss forward (BASELINE config 5) through the C ABI /
RetinaNetModel.get_loss vs the oracle restatement on identical inputs."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _model(loss_names, loss_weights):
    from bayes_od_rc_amd.model import RetinaNetModel
    cfg = {"output_names": ["classification", "regression", "regression_covar"], "mc_dropout_samples": 10,
           "header": {"dropout_rate": 0.3, "num_classes": 7, "anchors_per_location": 9},
           "losses": {"loss_names": loss_names, "loss_weights": loss_weights, "label_smoothing_epsilon": 0.001}}
    return RetinaNetModel(cfg)


@pytest.mark.parametrize("names,weights", [(["classification", "regression_covar"], [5.0, 1.0]),
                                           (["classification", "regression_var"], [5.0, 1.0]),
                                           (["classification", "regression"], [1.0, 50.0]),
                                           (["regression_covar"], [1.0])])
def test_get_loss_matches_oracle(names, weights):
    from test_losses_oracle import _sample
    from oracle import losses
    from bayes_od_rc_amd import constants
    rng = np.random.default_rng(5)
    sample, pred = _sample(rng, 3, 4911)
    sample32 = {constants.ANCHORS_KEY: sample["anchors"].astype(np.float32)[None],
                constants.POSITIVE_ANCHORS_MASK_KEY: sample["positive_anchors_mask"],
                constants.NEGATIVE_ANCHOR_MASK_KEY: sample["negative_anchors_mask"],
                constants.ANCHORS_CLASS_TARGETS_KEY: sample["anchors_class_targets"].astype(np.float32),
                constants.ANCHORS_BOX_TARGETS_KEY: sample["anchors_box_targets"].astype(np.float32)}
    pred32 = {k: v.astype(np.float32) for k, v in pred.items()}
    total, d = _model(names, weights).get_loss(sample32, pred32)
    # the oracle sees the same float32-rounded inputs, evaluated in float64
    s64 = {"anchors": sample32[constants.ANCHORS_KEY], "positive_anchors_mask": sample["positive_anchors_mask"],
           "negative_anchors_mask": sample["negative_anchors_mask"],
           "anchors_class_targets": sample32[constants.ANCHORS_CLASS_TARGETS_KEY],
           "anchors_box_targets": sample32[constants.ANCHORS_BOX_TARGETS_KEY]}
    ref_total, ref = losses.get_loss(s64, pred32, names, weights)
    assert abs(total - ref_total) <= 1e-3 * abs(ref_total)            # BASELINE.json: 1e-3 relative
    for k, v in ref.items():
        assert abs(d[k] - v) <= 1e-3 * abs(v) + 1e-9, k
    assert set(d) == set(ref)


def test_get_loss_errors():
    with pytest.raises(ValueError):
        _model(["bogus"], [1.0]).get_loss({}, {})


# ================================================================================================
# loss_kernel at its edges: both clamps of the box decode, the Huber switch, saturated logits, extreme log-variances, frames and
# calls without a positive, every (do_classification, reg_kind, label_smoothing), C = 4 and 8, shapes on the block edges
# ================================================================================================
EDGE_SHAPES = [(1, 1), (1, 255), (1, 256), (1, 257), (3, 171), (2, 3069)]       # (3, 171): a frame boundary inside a block
PLANTS = ("box_above_clamp", "box_below_clamp", "target_above_clamp", "target_below_clamp", "huber_plus_one", "huber_minus_one",
          "huber_inside", "huber_outside", "target_logit_high", "target_logit_low", "wrong_logit_high", "wrong_logit_low",
          "log_variance_high", "log_variance_low")
COV_DIAG = (4, 9, 5, 0)                    # fill_triangular: diagonal = (x4, x9, x5, x0)
_UNFILL = {4: (0, 0), 8: (1, 0), 9: (1, 1), 7: (2, 0), 6: (2, 1), 5: (2, 2), 3: (3, 0), 2: (3, 1), 1: (3, 2), 0: (3, 3)}
_edge_cache = {}


def edge_problem(b, a, c):
    """float32 inputs of one loss call from test_losses_oracle._sample, with PLANTS written onto positive anchors that sit on the
    edges of the 256-thread blocks and of the frames.  With b >= 2 the last frame has no positive.  Shared with the backward
    tests (tests/test_gpu_train_blocks.py); cached, never modified."""
    if (b, a, c) in _edge_cache:
        return _edge_cache[(b, a, c)]
    from test_losses_oracle import _sample
    f32 = np.float32
    rng = np.random.default_rng(1000 * b + 10 * a + c)
    sample, pred = _sample(rng, b, a, c)
    m = pred["anchors_box_covar_predictions"]
    p = {"b": b, "a": a, "c": c, "anchors": sample["anchors"].astype(f32),
         "pos": sample["positive_anchors_mask"].astype(np.uint8), "neg": sample["negative_anchors_mask"].astype(np.uint8),
         "cls_t": sample["anchors_class_targets"].astype(f32), "box_t": sample["anchors_box_targets"].astype(f32),
         "cls": pred["anchors_class_predictions"].astype(f32), "box": pred["anchors_box_predictions"].astype(f32),
         "cov": np.stack([m[..., _UNFILL[k][0], _UNFILL[k][1]] for k in range(10)], axis=-1).astype(f32)}
    last = b * a if b == 1 else (b - 1) * a                       # plants stay out of the frame without positives
    if b >= 2:
        p["pos"][b - 1] = 0
    want = [0, last - 1, 255, 256, a - 1, a, 511, 512, 2 * a - 1] + [int(x) for x in np.linspace(1, last - 2, 2 * len(PLANTS))]
    where = []
    for i in want:
        if 0 <= i < last and i not in where:
            where.append(i)
    where = where[:len(PLANTS)]
    flat = lambda k: p[k].reshape((b * a,) + p[k].shape[2:])
    plants = []
    for k, i in enumerate(where):
        kind, fg, wrong = PLANTS[k], k % (c - 1), (k + 1) % (c - 1)
        flat("pos")[i], flat("neg")[i] = 1, 0
        flat("cls_t")[i] = np.eye(c, dtype=f32)[fg]
        if kind == "box_above_clamp":                              # exp(z / 5) above 1e4, exp(w / 5) below 1e-4
            flat("box")[i, 2:] = (50.0, -50.0)
        elif kind == "box_below_clamp":
            flat("box")[i, 2:] = (-50.0, 50.0)
        elif kind == "target_above_clamp":
            flat("box_t")[i, 2:] = (50.0, -50.0)
        elif kind == "target_below_clamp":
            flat("box_t")[i, 2:] = (-50.0, 50.0)
        elif kind.startswith("huber"):                             # box - box_t exact in float32: +-1, and 2^-10 inside / outside
            d = {"huber_plus_one": 1.0, "huber_minus_one": -1.0, "huber_inside": 1.0 - 2.0 ** -10, "huber_outside": 1.0 + 2.0 ** -10}[kind]
            flat("box_t")[i] = (0.5, 0.25, -0.5, 0.125)
            flat("box")[i] = flat("box_t")[i] + np.array([d, -d, d, -d], f32)
        elif kind == "target_logit_high":
            flat("cls")[i, fg] = 80.0
        elif kind == "target_logit_low":
            flat("cls")[i, fg] = -80.0
        elif kind == "wrong_logit_high":
            flat("cls")[i, wrong if wrong != fg else c - 1] = 80.0
        elif kind == "wrong_logit_low":
            flat("cls")[i, wrong if wrong != fg else c - 1] = -80.0
        elif kind == "log_variance_high":
            flat("cov")[i, list(COV_DIAG)] = 8.0
        elif kind == "log_variance_low":
            flat("cov")[i, list(COV_DIAG)] = -8.0
        plants.append((kind, i))
    p["plants"] = plants
    _edge_cache[(b, a, c)] = p
    return p


def loss_modes():
    """(reg_kind, do_classification, label_smoothing): every regression kind with and without the focal term, both smoothings."""
    return [(rk, dc, eps) for rk in (0, 1, 2, 3) for dc, eps in ((0, 0.001), (1, 0.0), (1, 0.001))]


def oracle_terms(p, reg_kind, do_cls, eps, dtype, pos=None, neg=None):
    """Per-anchor terms [B,A] of the four sums (focal, regression, 0.5 sum log D, positives) from oracle.losses' own functions in
    `dtype`, as oracle.losses.get_loss composes them."""
    from oracle import geometry, losses, network
    t = dtype
    pos = (p["pos"] if pos is None else pos).astype(t)
    neg = (p["neg"] if neg is None else neg).astype(t)
    z = np.zeros(pos.shape, t)
    cls_term, cmp, reg = z, z, z
    if do_cls:
        cls_term = losses.softmax_focal_loss(p["cls_t"].astype(t), p["cls"].astype(t), gamma=2.0, label_smoothing=eps) * (pos + neg)
    if reg_kind == 1:
        cmp = losses.huber(p["box_t"].astype(t), p["box"].astype(t)).mean(axis=2) * pos
    elif reg_kind >= 2:
        anc = p["anchors"].astype(t)[None]
        pb = geometry.box_from_anchor_and_target(anc, p["box"].astype(t))
        tb = geometry.box_from_anchor_and_target(anc, p["box_t"].astype(t))
        cov = network.fill_triangular_4(p["cov"].astype(t))
        log_d = np.diagonal(cov, axis1=-2, axis2=-1)
        cmp = (np.exp(-log_d) * losses.huber(tb, pb)).sum(axis=2)
        if reg_kind == 3:
            l_inv = cov.copy()
            for i in range(4):
                l_inv[..., i, i] = 1.0
            cmp = np.sqrt((l_inv ** 2).sum(axis=(-2, -1))) * cmp
        cmp, reg = cmp * pos, t(0.5) * log_d.sum(axis=2) * pos
    return cls_term.astype(t), cmp.astype(t), reg.astype(t), pos


def device_loss_sums(p, reg_kind, do_cls, eps, pos=None, neg=None):
    import ctypes as C
    from bayes_od_rc_amd import _lib
    lib = _lib.load()
    pos = np.ascontiguousarray(p["pos"] if pos is None else pos, dtype=np.uint8)
    neg = np.ascontiguousarray(p["neg"] if neg is None else neg, dtype=np.uint8)
    out = (C.c_double * 4)()
    u8 = C.POINTER(C.c_uint8)
    st = lib.bod_loss_forward(0, p["b"], p["a"], p["c"], _lib.fptr(p["cls"]), _lib.fptr(p["cls_t"]), _lib.fptr(p["box"]),
                              _lib.fptr(p["box_t"]), _lib.fptr(p["cov"]), _lib.fptr(p["anchors"]), pos.ctypes.data_as(u8),
                              neg.ctypes.data_as(u8), int(do_cls), int(reg_kind), float(eps), out)
    _lib.check(lib, None, st)
    return np.array(list(out))


# (1 - p_t)^2 is exactly 0 in float32 once 1 - p_t < 2^-24 (a saturated target logit): up to 2^-48 * 0.5 * CE, CE <~ 170, is lost
# per anchor whatever the kernel does; nothing else in the four sums cancels
FOCAL_ABS = 1e-12
LOSS_REL_CAP = 1e-4


def loss_cases(p):
    """(label, reg_kind, do_cls, eps, pos, neg) of one problem: the modes on the problem's own masks, the call without a positive,
    and each planted anchor alone (masks that select only it)."""
    cases = [("all", rk, dc, eps, None, None) for rk, dc, eps in loss_modes()]
    nopos = np.zeros_like(p["pos"])
    cases += [("no_positive", 3, 1, 0.001, nopos, p["neg"]), ("no_positive", 1, 0, 0.001, nopos, p["neg"])]
    for kind, i in p["plants"]:
        only = np.zeros(p["b"] * p["a"], np.uint8)
        only[i] = 1
        only = only.reshape(p["b"], p["a"])
        for rk in (1, 2, 3):
            cases.append((kind + "_alone", rk, 1, 0.001, only, nopos))
        if "logit" in kind:
            cases.append((kind + "_alone", 0, 1, 0.0, only, nopos))
    return cases


def f32_oracle_worst():
    """The float32 oracle's worst error of a sum over EVERY case of every shape and class count below (the modes, the calls
    without a positive, each planted anchor alone), in units of the sum of the absolute per-anchor terms: the bound's yardstick,
    measured from the reference alone (about a second on the CPU, once per session)."""
    if "worst" not in _edge_cache:
        worst = 0.0
        for c in (4, 8):
            for b, a in EDGE_SHAPES:
                p = edge_problem(b, a, c)
                for _, rk, dc, eps, pos, neg in loss_cases(p):
                    t32 = oracle_terms(p, rk, dc, eps, np.float32, pos, neg)
                    worst = max(worst, sum_errors([x.sum(dtype=np.float32) for x in t32], p, rk, dc, eps, pos, neg)[0].max())
        _edge_cache["worst"] = float(worst)
    return _edge_cache["worst"]


def sum_errors(sums, p, reg_kind, do_cls, eps, pos, neg):
    """Error of four sums against the float64 oracle in units of the sum of the absolute per-anchor terms (the focal sum less
    FOCAL_ABS per masked anchor), and the float64 reference sums."""
    terms = oracle_terms(p, reg_kind, do_cls, eps, np.float64, pos, neg)
    ref = np.array([x.sum() for x in terms])
    scale = np.array([np.abs(x).sum() for x in terms[:3]])
    masked = float(((p["pos"] if pos is None else pos) | (p["neg"] if neg is None else neg)).sum())
    err = np.abs(np.asarray(sums[:3], np.float64) - ref[:3]) - np.array([FOCAL_ABS * masked, 0.0, 0.0])
    rel = np.where(scale > 0, np.maximum(err, 0.0) / np.where(scale > 0, scale, 1.0), np.where(err > 0, np.inf, 0.0))
    return rel, ref


@pytest.mark.parametrize("c", [4, 8])
@pytest.mark.parametrize("b,a", EDGE_SHAPES)
def test_loss_sums_at_the_edges(b, a, c):
    """The four sums of bod_loss_forward against oracle.losses in float64 for every case of loss_cases().  Each sum is within
    min(4 x f32_oracle_worst(), 1e-4) of the sum of its ABSOLUTE per-anchor terms (the log-determinant term is signed); the number
    of positives is exact.

    Measured: the float32 oracle's worst error is 5.32e-06 (one anchor alone, reg_kind 3: the Huber argument is a difference of
    two decoded boxes), which puts the bound at 2.13e-05; the device's worst on an MI355X is 5.55e-06 (shape (1, 256), C = 8)."""
    from oracle import losses, network
    p = edge_problem(b, a, c)
    assert len(p["plants"]) == min(len(PLANTS), b * a if b == 1 else (b - 1) * a)
    bound = min(4.0 * f32_oracle_worst(), LOSS_REL_CAP)
    assert 0.0 < bound <= LOSS_REL_CAP
    worst_dev = 0.0
    for label, rk, dc, eps, pos, neg in loss_cases(p):
        terms = oracle_terms(p, rk, dc, eps, np.float64, pos, neg)
        ref = np.array([x.sum() for x in terms])
        if label == "all":                                         # the per-anchor terms add up to oracle.losses.get_loss
            names = (["classification"] if dc else []) + ([[None, "regression", "regression_var", "regression_covar"][rk]] if rk else [])
            s64 = {"anchors": p["anchors"], "positive_anchors_mask": p["pos"], "negative_anchors_mask": p["neg"],
                   "anchors_class_targets": p["cls_t"], "anchors_box_targets": p["box_t"]}
            pr = {"anchors_class_predictions": p["cls"], "anchors_box_predictions": p["box"],
                  "anchors_box_covar_predictions": network.fill_triangular_4(p["cov"])}
            total, d = losses.get_loss(s64, pr, names, [1.0] * len(names), label_smoothing=eps)
            n = max(ref[3], 1.0)
            assert np.isclose(total * n, ref[:3].sum(), rtol=1e-12, atol=0)
            assert np.isclose(d.get("cls_loss", 0.0) * n, ref[0], rtol=1e-12, atol=0)
            assert np.isclose(d.get("reg_loss", 0.0) * n, ref[1], rtol=1e-12, atol=0)
        got = device_loss_sums(p, rk, dc, eps, pos, neg)
        rel, _ = sum_errors(got, p, rk, dc, eps, pos, neg)
        worst_dev = max(worst_dev, rel.max())
        assert got[3] == ref[3], (label, rk, dc, eps)
        assert rel.max() <= bound, (label, rk, dc, eps, rel, got, ref)
        if label == "no_positive":
            assert got[1] == 0.0 and got[2] == 0.0 and got[3] == 0.0
    print("loss sums (%d,%d) C=%d: device worst %.2e, bound %.2e (float32 oracle worst %.2e)" % (b, a, c, worst_dev, bound, f32_oracle_worst()))
