"""CPU: the host side of validation from ground-truth boxes -- the three entry points are declared everywhere the ABI is
declared, the loss assembly shared by get_loss and the batched route, the bucketing / flush / dataset-order logic of
run_validation with a fake engine, and the --batch option."""
import os
import re

import numpy as np
import pytest

from conftest import ANCHOR_CFG, ROOT

NAMES = ("bod_validation_losses_boxes", "bod_get_validation_detections_batch", "bod_validate_boxes")


def test_the_three_entry_points_are_declared():
    from bayes_od_rc_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bayesod.h")).read(), flags=re.S)
    cdef = open(os.path.join(ROOT, "include", "bayesod_cdef.h")).read()
    for name in NAMES:
        assert re.search(r"\bbod_status\s+%s\s*\(" % name, header), name
        assert re.search(r"\bbod_status\s+%s\s*\(" % name, cdef), name
        assert name in _lib.SIGNATURES
    # argument counts of the header and of the ctypes table agree
    for name in NAMES:
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, header).group(1)
        assert len(args.split(",")) == len(_lib.SIGNATURES[name][1]), name


def _get_loss_arithmetic(names, weights, s_cls, s_cmp, s_reg, n_pos):
    """retinanet_model.py:183-323 after the sums, written out independently: every term over max(n_pos, 1), the yaml weight
    on the classification and plain-regression entries, and on the total only for the variance / covariance losses."""
    d = max(n_pos, 1.0)
    w = dict(zip(names, weights))
    out, total = {}, 0.0
    if "classification" in w:
        out["cls_loss"] = w["classification"] * s_cls / d
        total += out["cls_loss"]
    if "regression" in w:
        out["reg_loss"] = w["regression"] * s_cmp / d
        total += out["reg_loss"]
    for n in ("regression_var", "regression_covar"):
        if n in w:
            out["reg_loss"], out["covariance_loss"] = s_cmp / d, s_reg / d
            total += w[n] * (s_cmp / d + s_reg / d)
    return total, out


@pytest.mark.parametrize("names,weights", [(["classification", "regression_covar"], [5.0, 1.0]),
                                           (["classification", "regression_var"], [5.0, 2.0]),
                                           (["classification", "regression"], [1.0, 50.0]),
                                           (["regression_covar"], [3.0])])
@pytest.mark.parametrize("sums", [(812.25, 96.5, -40.125, 166.0), (3.5, 0.0, 0.0, 0.0)])
def test_loss_assembly(names, weights, sums):
    from bayes_od_rc_amd.model import loss_from_sums
    total, d = loss_from_sums(names, weights, np.asarray(sums, np.float64))
    ref_total, ref = _get_loss_arithmetic(names, weights, *sums)
    assert set(d) == set(ref)
    assert abs(total - ref_total) <= 1e-12 * abs(ref_total)
    for k in ref:
        assert abs(d[k] - ref[k]) <= 1e-12 * abs(ref[k]), k
    if sums[3] == 0.0:                                     # no positives: divided by 1
        assert d.get("cls_loss", 0.0) == (weights[names.index("classification")] * sums[0] if "classification" in names else 0.0)
        assert d["reg_loss"] == 0.0


def test_regularization_loss_covers_the_trained_head_kernels():
    from bayes_od_rc_amd.model import RetinaNetModel
    cfg = {"output_names": ["classification", "regression", "regression_covar"], "mc_dropout_samples": 10,
           "header": {"dropout_rate": 0.3, "num_classes": 7, "anchors_per_location": 9, "l2_norm_rate": "1e-3"},
           "losses": {"loss_names": ["classification", "regression_covar"], "loss_weights": [5.0, 1.0]}}
    rng = np.random.default_rng(0)
    layers = (["pyramid_classification_%d" % i for i in range(4)] + ["pyramid_regression_%d" % i for i in range(4)]
              + ["pyramid_cov_%d" % i for i in range(4)] + ["pyramid_classification", "pyramid_regression", "pyramid_cov", "P3"])
    weights = {l: {"kernel": rng.normal(size=(3, 3, 4, 4)).astype(np.float32), "bias": np.ones(4, np.float32)} for l in layers}
    model = RetinaNetModel(cfg)
    with pytest.raises(ValueError):
        model.regularization_loss()
    model.load_weights(weights)
    used = [l for l in layers if re.search(r"_\d$", l) and l != "pyramid_regression_3"] + ["pyramid_cov"]
    want = 1e-3 * sum(float((weights[l]["kernel"].astype(np.float64) ** 2).sum()) for l in used)
    assert abs(model.regularization_loss() - want) <= 1e-12 * want
    assert model.loss_kinds() == (True, 3)
    cfg2 = dict(cfg, output_names=["classification", "regression"])
    model2 = RetinaNetModel(cfg2)
    model2.load_weights(weights)
    want2 = 1e-3 * sum(float((weights[l]["kernel"].astype(np.float64) ** 2).sum()) for l in used if "cov" not in l)
    assert abs(model2.regularization_loss() - want2) <= 1e-12 * want2


class _FakeEngine(object):
    """Stands in for the handle: records what it was asked and answers with values that name the frame."""

    def __init__(self, batch, log):
        self.B, self.log, self._anchors_set = batch, log, False

    def set_anchors(self, anchors):
        self._anchors_set = True

    def upload_frames_u8(self, frames, means, aspect_resize=False):
        assert frames.shape[0] == self.B and frames.dtype == np.uint8
        self.tags = [int(f[0, 0, 0]) for f in frames]
        self.log.append(("upload", self.B, frames.shape[1:3], bool(aspect_resize)))

    def validate_boxes(self, images, gt_boxes, gt_classes, min_positive_iou, max_negative_iou, do_classification, reg_kind,
                       label_smoothing):
        assert images is None and len(gt_boxes) == self.B == len(gt_classes)
        assert (min_positive_iou, max_negative_iou, do_classification, reg_kind) == (0.5, 0.4, True, 3)
        self.log.append(("validate", tuple(self.tags)))
        sums = np.asarray([[10.0 * (t + 1), 2.0, 1.0, 2.0] for t in self.tags])
        dets = [(np.tile(np.eye(8, dtype=np.float32)[0] * 0.5, (t + 1, 1)), np.full((t + 1, 4), float(t), np.float32)) for t in self.tags]
        return sums, dets


class _FakeModel(object):
    def __init__(self, log):
        self.log, self.engines = log, {}

    def engine_for(self, hw, batch=None, mc_samples=None, **kw):
        from bayes_od_rc_amd.run_validation import VALIDATION_NMS
        assert mc_samples == 1 and kw == {"nms_config": VALIDATION_NMS}
        return self.engines.setdefault((tuple(hw), batch), _FakeEngine(batch, self.log))

    def loss_kinds(self):
        return True, 3

    def regularization_loss(self):
        return 0.25


def _samples(sizes):
    """Ground-truth-only samples; pixel (0, 0) carries the frame's position in the dataset."""
    from bayes_od_rc_amd.sample_builder import create_sample_dict
    out = []
    for i, hw in enumerate(sizes):
        sample = create_sample_dict(np.zeros(hw + (3,), np.float32), ANCHOR_CFG, np.asarray([[4.0, 4.0, 40.0, 40.0]], np.float32),
                                    np.eye(8, dtype=np.float32)[:1], dense_targets=False)
        sample["image_uint8"] = np.full(hw + (3,), i, np.uint8)
        out.append(sample)
    return out


def test_bucketing_flush_and_dataset_order():
    from bayes_od_rc_amd import run_validation
    from bayes_od_rc_amd.run_training import bucket_minibatches
    a, b = (64, 64), (64, 96)
    sizes = [a, b, a, a, b, a, b, a]                       # size a: frames 0 2 3 5 7, size b: frames 1 4 6
    config = {"dataset_config": {"dataset": "bdd", "anchor_generator": ANCHOR_CFG, "im_normalization": "ImageNet"},
              "model_config": {"losses": {"loss_names": ["classification", "regression_covar"], "loss_weights": [5.0, 1.0]}}}
    log = []
    ids = ["f%d.jpg" % i for i in range(len(sizes))]
    records, totals, sums, ndet = run_validation._validate_batched(_FakeModel(log), config, iter(_samples(sizes)), ids, None,
                                                                   ["car"] * 7, 3)
    # full buckets as they fill, then the partial ones as tail batches through handles of their own size
    assert [e[1] for e in log if e[0] == "validate"] == [(0, 2, 3), (1, 4, 6), (5, 7)]
    assert [e[1:3] for e in log if e[0] == "upload"] == [(3, a), (3, b), (2, a)]
    assert not any(e[3] for e in log if e[0] == "upload")              # BDD frames are not resized
    # per-frame losses from the frame's own sums (n_pos = 2), regularisation added; dataset order restored
    assert totals == [5.0 * 10.0 * (i + 1) / 2.0 + (2.0 + 1.0) / 2.0 + 0.25 for i in range(len(sizes))]
    assert abs(sums["regularization_loss"] - 0.25 * len(sizes)) < 1e-12 and abs(sums["reg_loss"] - len(sizes)) < 1e-12
    assert [r["name"] for r in records] == [ids[i] for i in range(len(sizes)) for _ in range(i + 1)]
    assert ndet == sum(i + 1 for i in range(len(sizes))) == len(records)
    assert all(r["bbox"] == [float(ids.index(r["name"]))] * 4 for r in records)
    # flush_buckets empties the carry and cuts buckets larger than a batch
    carry = {}
    assert list(bucket_minibatches(iter(_samples([a] * 2 + [b])), 5, carry)) == []
    carry[a] = carry[a] * 3
    tails = list(run_validation.flush_buckets(carry, 4))
    assert [len(t) for t in tails] == [4, 2, 1] and carry == {}


def test_kitti_batches_are_resized_on_the_device_and_rescaled_on_the_host(tmp_path):
    from bayes_od_rc_amd import constants, run_validation
    config = {"dataset_config": {"dataset": "kitti", "anchor_generator": ANCHOR_CFG, "im_normalization": "ImageNet",
                                 "kitti": {"resize_shape": [64, 128]}},
              "model_config": {"losses": {"loss_names": ["classification", "regression_covar"], "loss_weights": [5.0, 1.0]}}}
    log = []
    samples = _samples([(64, 128)] * 2)
    for s in samples:
        s[constants.IMAGE_NORMALIZED_KEY] = None
        s["image_uint8"] = np.full((32, 96, 3), s["image_uint8"][0, 0, 0], np.uint8)
        s[constants.ORIGINAL_IM_SIZE_KEY] = np.asarray([32, 96, 3], np.int32)
    out = run_validation.validate_batch(_FakeModel(log), config, samples)
    assert log[0] == ("upload", 2, (32, 96), True)
    n, s = np.asarray([64, 128] * 2, np.float32), np.asarray([32, 96] * 2, np.float32)
    assert np.array_equal(out[1][3], (np.full((2, 4), 1.0, np.float32) / n) * s)
    records, totals, sums, ndet = run_validation._validate_batched(_FakeModel([]), config, iter(samples), ["000000", "000001"],
                                                                   str(tmp_path), None, 8)
    assert records == [] and ndet == 3 and sorted(os.listdir(str(tmp_path))) == ["000000.txt", "000001.txt"]


def test_batch_option(monkeypatch, tmp_path):
    from bayes_od_rc_amd import run_validation
    monkeypatch.setenv("BAYESOD_DATA_DIR", str(tmp_path))               # config_utils.setup creates the run's output folders
    seen = {}

    def fake_validate(config, samples, sample_ids, **kw):
        seen.update(kw, n=len(sample_ids))
        return []
    monkeypatch.setattr(run_validation, "validate", fake_validate)
    monkeypatch.setattr(run_validation, "RetinaNetModel", None)
    import bayes_od_rc_amd.run_training as rt
    monkeypatch.setattr(rt, "synthetic_samples", lambda n, *a, **k: [{}] * n)
    assert run_validation.main(["--synthetic", "2"]) == [] and seen["batch"] == 8 and seen["n"] == 2
    assert run_validation.main(["--synthetic", "2", "--batch", "3"]) == [] and seen["batch"] == 3
    with pytest.raises(SystemExit):
        run_validation.main(["--batch", "0"])
    with pytest.raises(SystemExit):
        run_validation.main(["--batch", "many"])
