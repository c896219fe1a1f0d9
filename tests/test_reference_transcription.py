"""CPU: oracle/bayes_od.py against vectors produced by the reference's OWN ``bayes_od_inference`` source
(src/retina_net/experiments/inference_utils.py:13-217) executed under a NumPy stand-in for TensorFlow
(tests/tools/tf_numpy_shim.py, tests/golden/make_transcription_golden.py -> tests/golden/reference_transcription.npz).

This is a TRANSCRIPTION check: formulas, axes, mixing weights and branches of the reference function as written.  It does not
pin TensorFlow's op semantics (stand-ins), the categorical sampler (the oracle's injected uniforms) or the soft-NMS
(oracle/nms.py is what the stand-in calls): the oracle stays "parity unpinned" for SURVEY rows a1-a15."""
import os
import sys

import numpy as np
import pytest

from oracle import bayes_od, geometry, losses, nms, validation

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "reference_transcription.npz")
sys.path.insert(0, os.path.join(HERE, "golden"))


def _cases():
    import make_transcription_golden as gen
    return gen.CASES


@pytest.mark.parametrize("case", _cases(), ids=[c[0] for c in _cases()])
def test_oracle_posterior_equals_the_reference_source_run_under_the_numpy_stand_in(case):
    name, n, a, c, covar, full, dirich, gauss, ranking, dataset = case
    z = np.load(GOLDEN)
    pred = {k: z["%s.in.%s" % (name, k)].astype(np.float64)
            for k in ("anchors_class_predictions", "anchors_box_predictions", "anchors_box_covar_predictions") if "%s.in.%s" % (name, k) in z.files}
    assert ("anchors_box_covar_predictions" in pred) == covar
    anchors, uniforms = z[name + ".in.anchors"].astype(np.float64), z[name + ".in.uniforms"].astype(np.float64)
    cfg = {"ranking_method": ranking, "dirichlet_prior": {"type": dirich}, "gaussian_prior": {"type": gauss, "isotropic_variance": 100000.0}}
    net = (384, 1248, 3) if dataset == "kitti" else (512, 512, 3)
    out = bayes_od.bayes_od_posterior(pred, anchors, uniforms, cfg, use_full_covar=full, dataset_name=dataset, orig_size=(375, 1242, 3),
                                      net_size=net, dtype=np.float64)
    counts, means, covs = z[name + ".out.counts"], z[name + ".out.means"], z[name + ".out.covs"]
    assert out["counts"].shape == counts.shape and 0 < counts.shape[0] < a            # some anchors filtered as background, some kept
    assert np.array_equal(out["counts"], counts)                                      # Dirichlet posterior counts: exact
    np.testing.assert_allclose(out["means"], means, rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(out["covs"], covs, rtol=1e-9, atol=1e-12)
    # bbox_iou_vuvu of the posterior corners with themselves (the affinity matrix of the clustering stage)
    np.testing.assert_allclose(geometry.bbox_iou_vuvu(out["corners"], out["corners"]), z[name + ".out.iou"], rtol=1e-9, atol=1e-12)
    # the ranking scores (max posterior score or the joint-entropy information gain) order the soft-NMS: same centres, same order
    idx = nms.soft_nms(out["corners"], out["ranking"], max_output_size=100, iou_threshold=0.5, soft_nms_sigma=0.5)[0]
    assert np.array_equal(np.asarray(idx), z[name + ".out.nms"])


def _loss_cases():
    import make_transcription_golden as gen
    return gen.LOSS_CASES


@pytest.mark.parametrize("case", _loss_cases(), ids=[c[0] for c in _loss_cases()])
def test_oracle_loss_equals_the_reference_get_loss_run_under_the_numpy_stand_in(case):
    """RetinaNetModel.get_loss (retinanet_model.py:151-328) + SoftmaxFocalLoss.call (src/core/losses.py:30-61), executed from the
    reference's source on a bare object (no network), against oracle/losses.py: the focal term, the three regression kinds
    (Huber on targets; Huber on decoded boxes weighted by exp(-log D), without / with the Frobenius norm of the unit-diagonal L),
    the normalisation by max(1, positives) and a batch without positives."""
    name, b, a, c, names, weights = case
    z = np.load(GOLDEN)
    g = lambda k: z["%s.in.%s" % (name, k)].astype(np.float64)
    sample = {k: g(k) for k in ("anchors", "positive_anchors_mask", "negative_anchors_mask", "anchors_class_targets", "anchors_box_targets")}
    pred = {k: g(k) for k in ("anchors_class_predictions", "anchors_box_predictions", "anchors_box_covar_predictions")}
    total, parts = losses.get_loss(sample, pred, names, weights, label_smoothing=0.001, dtype=np.float64)
    want = {k.split(".out.")[1]: float(z[k]) for k in z.files if k.startswith(name + ".out.")}
    assert set(parts) | {"total"} == set(want), (sorted(parts), sorted(want))
    for k, v in parts.items():
        assert abs(float(v) - want[k]) <= 1e-10 * max(1.0, abs(want[k])), (k, float(v), want[k])
    # (the reference accumulates total_loss from tf.constant(0.0), a float32)
    assert abs(float(total) - want["total"]) <= 2e-6 * max(1.0, abs(want["total"])), (float(total), want["total"])
    if "nopos" in name:
        assert want["reg_loss"] == 0.0 and want["cls_loss"] > 0


def _forward_cases():
    import make_transcription_golden as gen
    return gen.FORWARD_CASES


@pytest.mark.parametrize("case", _forward_cases(), ids=[c[0] for c in _forward_cases()])
def test_oracle_forward_equals_the_reference_model_wiring_run_under_the_layer_stand_ins(case):
    """RetinaNetModel.__init__ + call('testing') with FeatureExtractor / ConvBlock / IdentityBlock, FeatureDecoder and the three
    headers CONSTRUCTED AND CALLED from the reference's source (retinanet_model.py:18-112, feature_extractor.py, feature_decoder.py,
    multitask_headers.py), Keras layers standing in with oracle/network.py's primitives and the oracle's Philox masks: checks the
    wiring of oracle/network.py -- block order and strides, the taps, the FPN merges (m4 is upsampled into p3, not p4), P6 from C5
    and P7 from relu(P6), RegHeader's three convolutions, MC tiling, dropout placement and on/off rule, the anchor-major reshape /
    level concat, fill_triangular -- not the primitives themselves."""
    import make_transcription_golden as gen
    from oracle import network
    name, hw, n, seed = case
    z = np.load(GOLDEN)
    weights, frame = gen.forward_inputs(hw, seed)
    km, _ = gen.forward_masks(hw, n)
    out = network.retinanet_forward(weights, frame, n, 8, mode="literal", dtype=np.float64, keep_masks=km)
    for k in ("anchors_class_predictions", "anchors_box_predictions", "anchors_box_covar_predictions"):
        want = z["%s.out.%s" % (name, k)].astype(np.float64)
        assert out[k].shape == want.shape, (k, out[k].shape, want.shape)
        assert np.abs(want).max() > 0
        np.testing.assert_allclose(out[k], want, rtol=2e-6, atol=2e-6 * np.abs(want).max())
    if n > 1:                      # MC samples differ (dropout on) ...
        assert np.abs(out["anchors_class_predictions"][0] - out["anchors_class_predictions"][1]).max() > 1e-3
    # ... and with one sample the reference turns dropout off: compare with a second evaluation without masks
    if n == 1:
        again = network.retinanet_forward(weights, frame, 1, 8, mode="literal", dtype=np.float64, keep_masks=None)
        assert np.array_equal(again["anchors_box_predictions"], out["anchors_box_predictions"])


@pytest.mark.parametrize("dataset", ["bdd", "kitti"])
def test_oracle_validation_post_process_equals_the_reference_source(dataset):
    """validation_utils.post_process_predictions (:10-77) from the reference's source against oracle/validation.py."""
    z = np.load(GOLDEN)
    name = "val_" + dataset
    anchors = z[name + ".in.anchors"].astype(np.float64)
    cls, box = z[name + ".in.anchors_class_predictions"].astype(np.float64)[0], z[name + ".in.anchors_box_predictions"].astype(np.float64)[0]
    net = (384, 1248) if dataset == "kitti" else (512, 512)
    classes, corners, info = validation.post_process_predictions(anchors, box, cls, dataset_name=dataset, net_hw=net, orig_hw=(375, 1242), dtype=np.float64)
    want_c, want_b = z[name + ".out.classes"], z[name + ".out.corners"]
    assert classes.shape == want_c.shape and 0 < want_c.shape[0] < anchors.shape[0]
    np.testing.assert_allclose(classes, want_c, rtol=1e-12, atol=1e-15)
    # (the reference casts the image / original sizes to float32 before dividing: 1e-6 on the KITTI rescale)
    np.testing.assert_allclose(corners, want_b, rtol=1e-6 if dataset == "kitti" else 1e-12, atol=1e-9)


def test_training_oracle_forward_equals_the_reference_training_mode_call():
    """RetinaNetModel.call(x, 'training') (retinanet_model.py:113-147) from the reference's source on two frames against
    oracle/torch_train.forward -- the PyTorch restatement under the training step's autograd oracle (f1): dropout on at one pass
    over the un-tiled batch, literal BatchNorm in inference mode, same Philox masks."""
    import torch
    from bayes_od_rc_amd import synthetic
    from oracle import network, torch_train
    z = np.load(GOLDEN)
    weights = synthetic.make_weights(cls_fg_bias=-2.0)
    frames = synthetic.make_frames(2, 64, 64, seed=5)
    tw, _ = torch_train.prepare(weights, torch.float64)
    with torch.no_grad():
        cls, box, cov = torch_train.forward(tw, frames, 3, 10, 8, dtype=torch.float64)
    got = {"anchors_class_predictions": cls.numpy(), "anchors_box_predictions": box.numpy(),
           "anchors_box_covar_predictions": network.fill_triangular_4(cov.numpy())}
    for k, v in got.items():
        want = z["train_fwd.out." + k].astype(np.float64)
        assert v.shape == want.shape, (k, v.shape, want.shape)
        np.testing.assert_allclose(v, want, rtol=2e-6, atol=2e-6 * np.abs(want).max())


def test_the_gaussian_prior_none_branch_of_the_reference_raises():
    """Finding of the transcription run, kept as data (tests/golden/reference_findings.json, written by make_transcription_golden.py):
    with gaussian_prior 'None' the reference keeps the likelihood means rank 2 and its own tf.squeeze(..., axis=2) (:204-205) raises.
    The build returns the likelihood instead (test_bayes_oracle.py): on the same inputs the oracle's likelihood means are rank 2 as
    well, and its posterior is that likelihood."""
    import json
    import make_transcription_golden as gen
    with open(os.path.join(HERE, "golden", "reference_findings.json")) as fp:
        rec = json.load(fp)["gaussian_prior_none"]
    assert rec["raised"] == "AxisError" and rec["means_rank"] == 2, rec
    assert rec["config"] == gen.GAUSSIAN_NONE_CFG and rec["make_inputs"] == gen.GAUSSIAN_NONE_INPUTS
    pred, anchors, u = gen.make_inputs(*rec["make_inputs"])
    out = bayes_od.bayes_od_posterior(pred, anchors, u, rec["config"], use_full_covar=rec["use_full_covar"], dataset_name=rec["dataset"],
                                      dtype=np.float64, return_debug=True)
    m = int(out["keep"].sum())
    assert m > 0 and out["mu"].shape == (m, 4) and out["mu"].ndim == rec["means_rank"]
    assert out["means"].shape == (m, 4, 1) and np.array_equal(out["means"][:, :, 0], out["mu"])
    assert np.array_equal(out["covs"], out["cov_lik"])
