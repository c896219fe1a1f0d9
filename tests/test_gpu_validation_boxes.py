"""GPU: validation from ground-truth boxes -- per-frame loss sums on device-resident outputs and targets
(bod_validation_losses_boxes), the gathered detection records (bod_get_validation_detections_batch), the whole step
(bod_validate_boxes) and run_validation --dataset on a BDD-shaped and a KITTI tree.

Inputs: 128x160 with conftest.ANCHOR_CFG (A = 3852).  Frame b's raw outputs come from default_rng(3 + b) -- frame 0 is the input of
test_gpu_post.py::test_validation_post_process_matches_oracle -- and its ground truth from the recipe of
test_gpu_train_from_boxes.py::_gt_from_anchors with seed b (166, 203, 192 positives on the host generator); a fourth frame
carries the placeholder row (no positives, every anchor negative)."""
import gc
import json
import os
import weakref

import numpy as np
import pytest

from conftest import ANCHOR_CFG, NMS_CFG

pytestmark = pytest.mark.gpu

HW = (128, 160)
LOSS_CONFIGS = [(["classification", "regression_covar"], [5.0, 1.0]), (["classification", "regression_var"], [5.0, 1.0]),
                (["classification", "regression"], [1.0, 50.0]), (["regression_covar"], [1.0])]          # those of test_gpu_loss.py
REG_KIND = {"regression": 1, "regression_var": 2, "regression_covar": 3}


def _kinds(names):
    reg = [n for n in names if n in REG_KIND]
    return "classification" in names, (REG_KIND[reg[0]] if reg else 0)


class Problem(object):
    pass


@pytest.fixture(scope="module")
def problem():
    from bayes_od_rc_amd.anchor_generator import FpnAnchorGenerator
    from bayes_od_rc_amd.engine import anchor_targets
    from test_gpu_train_from_boxes import _gt_from_anchors
    p = Problem()
    p.anchors = FpnAnchorGenerator(ANCHOR_CFG).generate_all(HW + (3,)).astype(np.float32)
    a = p.anchors.shape[0]
    assert a == 3852
    p.cls, p.box, p.cov = [], [], []
    for b in range(4):
        rng = np.random.default_rng(3 + b)
        logits = rng.normal(0, 1.5, (a, 8)).astype(np.float32)
        logits[:, 7] += 1.0                                           # background wins for most anchors
        p.cls.append(logits)
        p.box.append(rng.normal(0, 0.6, (a, 4)).astype(np.float32))
        p.cov.append(rng.normal(0, 0.5, (a, 10)).astype(np.float32))
    gt = [_gt_from_anchors(p.anchors, seed) for seed in range(3)]
    gt.append((np.asarray([[0.0, 0.0, 1.0, 1.0]], np.float32), np.eye(8, dtype=np.float32)[7:8]))      # the handlers' placeholder row
    p.gt_boxes, p.gt_classes = [g[0] for g in gt], [g[1] for g in gt]
    # the targets the device assigns (pinned to NumPy by test_gpu_anchor_targets.py)
    p.cls_t, p.box_t, p.pos, p.neg = anchor_targets(p.anchors, p.gt_boxes, p.gt_classes, 0.5, 0.4)
    n_pos = p.pos.sum(axis=1)
    print("positives per frame:", n_pos.tolist())
    assert (n_pos[:3] >= 50).all() and n_pos[3] == 0 and p.neg[3].all()
    for arr in (p.anchors, p.cls_t, p.box_t, p.pos, p.neg, *p.cls, *p.box, *p.cov):
        arr.setflags(write=False)
    return p


def _engine(batch, **kw):
    from bayes_od_rc_amd.engine import Engine, make_config
    return Engine(make_config(HW, batch=batch, mc_samples=1, nms_config=NMS_CFG, **kw))


def _set(eng, p, order):
    eng.set_raw(np.stack([p.cls[f] for f in order])[:, None], np.stack([p.box[f] for f in order])[:, None],
                np.stack([p.cov[f] for f in order])[:, None])


def _losses(eng, p, order, do_cls=True, kind=3):
    return eng.validation_losses_boxes([p.gt_boxes[f] for f in order], [p.gt_classes[f] for f in order], 0.5, 0.4,
                                       do_classification=do_cls, reg_kind=kind, label_smoothing=0.001)


@pytest.fixture(scope="module")
def batch4(problem):
    eng = _engine(4)
    eng.set_anchors(problem.anchors)
    _set(eng, problem, range(4))
    yield eng
    eng.close()


@pytest.mark.parametrize("names,weights", LOSS_CONFIGS)
def test_loss_sums_match_the_oracle(problem, batch4, names, weights):
    """Each frame's total and loss-dict entries within 1e-3 relative of oracle.losses.get_loss (float64 on the same float32
    inputs and the same assigned targets): BASELINE's bound, the one test_gpu_loss.py uses."""
    from bayes_od_rc_amd.model import fill_triangular_4, loss_from_sums
    from oracle import losses
    p = problem
    do_cls, kind = _kinds(names)
    sums = _losses(batch4, p, range(4), do_cls, kind)
    assert sums.shape == (4, 4) and sums.dtype == np.float64
    assert np.array_equal(sums[:, 3], p.pos.sum(axis=1))
    for f in range(4):
        total, d = loss_from_sums(names, weights, sums[f])
        sample = {"anchors": p.anchors, "positive_anchors_mask": p.pos[f:f + 1], "negative_anchors_mask": p.neg[f:f + 1],
                  "anchors_class_targets": p.cls_t[f:f + 1], "anchors_box_targets": p.box_t[f:f + 1]}
        pred = {"anchors_class_predictions": p.cls[f][None], "anchors_box_predictions": p.box[f][None],
                "anchors_box_covar_predictions": fill_triangular_4(p.cov[f][None])}
        ref_total, ref = losses.get_loss(sample, pred, names, weights)
        print(f, total, ref_total, d, ref)
        assert abs(total - ref_total) <= 1e-3 * abs(ref_total)
        assert set(d) == set(ref)
        for k, v in ref.items():
            assert abs(d[k] - v) <= 1e-3 * abs(v) + 1e-9, (f, k)
    # the placeholder frame: a finite classification loss divided by 1, no regression / covariance terms
    total, d = loss_from_sums(names, weights, sums[3])
    assert sums[3, 1] == 0.0 and sums[3, 2] == 0.0 and d["reg_loss"] == 0.0 and d.get("covariance_loss", 0.0) == 0.0
    if do_cls:
        assert np.isfinite(d["cls_loss"]) and d["cls_loss"] > 0 and d["cls_loss"] == sums[3, 0] * weights[names.index("classification")]


@pytest.mark.parametrize("kind", [1, 2, 3])
def test_loss_sums_match_bod_loss_forward(problem, batch4, kind):
    """Each frame's four sums against bod_loss_forward on that frame alone with the same targets: 1e-5 |ref| + 1e-7, the bound
    test_gpu_train_from_boxes.py holds two routes of the same arithmetic to that differ only in the order of their sums."""
    import ctypes as C
    from bayes_od_rc_amd import _lib
    p = problem
    lib = _lib.load()
    u8 = C.POINTER(C.c_uint8)
    sums = _losses(batch4, p, range(4), True, kind)
    for f in range(4):
        out = (C.c_double * 4)()
        pos, neg = p.pos[f].astype(np.uint8), p.neg[f].astype(np.uint8)
        cls_t, box_t = np.ascontiguousarray(p.cls_t[f]), np.ascontiguousarray(p.box_t[f])
        st = lib.bod_loss_forward(0, 1, p.anchors.shape[0], 8, _lib.fptr(p.cls[f]), _lib.fptr(cls_t), _lib.fptr(p.box[f]), _lib.fptr(box_t),
                                  _lib.fptr(p.cov[f]), _lib.fptr(p.anchors), pos.ctypes.data_as(u8), neg.ctypes.data_as(u8), 1, kind,
                                  0.001, out)
        _lib.check(lib, None, st)
        print(f, kind, list(sums[f]), list(out))
        for q in range(4):
            assert abs(sums[f, q] - out[q]) <= 1e-5 * abs(out[q]) + 1e-7, (f, q, sums[f, q], out[q])


def test_a_frames_sums_do_not_depend_on_its_batch_or_position(problem, batch4):
    """Bitwise: the four rotations of the batch put every frame at every position (0 and 3 included); then alone in a batch-1
    handle."""
    p = problem
    ref = _losses(batch4, p, range(4))
    eng = _engine(4)
    eng.set_anchors(p.anchors)
    for r in range(1, 4):
        order = [(i + r) % 4 for i in range(4)]
        _set(eng, p, order)
        got = _losses(eng, p, order)
        for pos, f in enumerate(order):
            assert np.array_equal(got[pos], ref[f]), (r, pos, f, got[pos], ref[f])
    eng.close()
    one = _engine(1)
    one.set_anchors(p.anchors)
    for f in range(4):
        _set(one, p, [f])
        got = _losses(one, p, [f])
        assert got.shape == (1, 4) and np.array_equal(got[0], ref[f]), (f, got, ref[f])
    one.close()


@pytest.mark.parametrize("dataset", ["bdd", "kitti"])
def test_detections_match_post_process_predictions(problem, batch4, dataset):
    """validation_post + nms + the batch getter on the batch against inference_utils.post_process_predictions on each frame
    alone (same kernels, same inputs): array_equal.  Frame 0 also against the oracle under the existing test's bounds."""
    from bayes_od_rc_amd import constants, inference_utils, run_validation
    from oracle import validation
    p = problem
    orig = (375, 1242)
    _set(batch4, p, range(4))
    batch4.validation_post()
    batch4.nms()
    dets = batch4.validation_detections_batch()
    assert len(dets) == 4
    one = _engine(1)
    one.set_anchors(p.anchors)
    for f in range(4):
        sample = {constants.ANCHORS_KEY: p.anchors[None], constants.IMAGE_NORMALIZED_KEY: np.zeros((1,) + HW + (3,), np.float32),
                  constants.ORIGINAL_IM_SIZE_KEY: np.asarray([[orig[0], orig[1], 3]], np.int32)}
        pred = {constants.ANCHORS_CLASS_PREDICTIONS_KEY: p.cls[f][None], constants.ANCHORS_BOX_PREDICTIONS_KEY: p.box[f][None]}
        ref_classes, ref_corners = inference_utils.post_process_predictions(sample, pred, dataset_name=dataset, engine=one)
        classes, corners = dets[f]
        if dataset == "kitti":
            corners = run_validation.kitti_rescale(corners, HW, sample[constants.ORIGINAL_IM_SIZE_KEY])
        assert classes.dtype == ref_classes.dtype and corners.dtype == ref_corners.dtype
        assert np.array_equal(classes, ref_classes) and np.array_equal(corners, ref_corners), f
        if f < 3:
            assert len(classes) == 100            # (the oracle keeps 2780 / 2790 / 2750 anchors and selects 100 on each)
    one.close()
    classes, corners = dets[0]
    if dataset == "kitti":
        corners = run_validation.kitti_rescale(corners, HW, [orig[0], orig[1], 3])
    ref_c, ref_b, info = validation.post_process_predictions(p.anchors, p.box[0], p.cls[0], dataset_name=dataset, net_hw=HW, orig_hw=orig,
                                                             dtype=np.float32)
    assert 50 < info["keep"].sum() < p.anchors.shape[0] and len(info["nms"]) == 100
    assert classes.shape == ref_c.shape and corners.shape == ref_b.shape
    assert np.abs(classes - ref_c).max() < 1e-5
    assert np.abs(corners - ref_b).max() < 1e-3 * max(1.0, float(np.abs(ref_b).max()))


# cls_fg_bias of the synthetic weights for the tests with a real forward: see test_whole_step_equals_the_staged_calls
FG_BIAS = -1.0


def test_whole_step_equals_the_staged_calls(problem):
    """validate_boxes == forward + validation_losses_boxes + validation_post + nms + the batch getter, bit for bit, on the same
    handle and frames; the regularisation term equals the one a training handle reports for the same weights and l2_rate.
    Non-vacuity: with synthetic.make_weights' default class bias (-4.6), and with -2.0, the background wins on every anchor of
    these frames (no detection); cls_fg_bias = -1.0 keeps 683 and 626 anchors and selects 100 detections on each frame."""
    from bayes_od_rc_amd import synthetic
    from bayes_od_rc_amd.engine import Engine, make_config
    from bayes_od_rc_amd.model import RetinaNetModel
    p = problem
    weights = synthetic.make_weights(cls_fg_bias=FG_BIAS)
    frames = synthetic.make_frames(2, HW[0], HW[1], seed=5)
    boxes, classes = p.gt_boxes[:2], p.gt_classes[:2]
    eng = _engine(2)
    eng.load_weights(weights)
    eng.set_anchors(p.anchors)
    sums, dets = eng.validate_boxes(frames, boxes, classes, 0.5, 0.4)
    eng.forward(frames)
    staged_sums = eng.validation_losses_boxes(boxes, classes, 0.5, 0.4)
    eng.validation_post()
    eng.nms()
    staged = eng.validation_detections_batch()
    print("sums", sums.tolist(), "detections per frame", [len(d[1]) for d in dets])
    assert np.isfinite(sums).all() and np.array_equal(sums, staged_sums)
    assert np.array_equal(sums[:, 3], p.pos[:2].sum(axis=1))
    for (c0, b0), (c1, b1) in zip(dets, staged):
        assert np.array_equal(c0, c1) and np.array_equal(b0, b1)
    assert max(len(d[1]) for d in dets) >= 1 and all(len(d[0]) == len(d[1]) for d in dets)
    # frames already on the device
    eng.upload_images(frames)
    sums_dev, dets_dev = eng.validate_boxes(None, boxes, classes, 0.5, 0.4)
    assert np.array_equal(sums_dev, sums) and all(np.array_equal(x[1], y[1]) for x, y in zip(dets_dev, dets))
    eng.close()
    # regularisation: Keras l2(rate) over the tensors the training step regularises
    cfg = {"output_names": ["classification", "regression", "regression_covar"], "mc_dropout_samples": 10,
           "header": {"dropout_rate": 0.3, "num_classes": 7, "anchors_per_location": 9, "l2_norm_rate": 1e-6},
           "losses": {"loss_names": ["classification", "regression_covar"], "loss_weights": [5.0, 1.0]}}
    model = RetinaNetModel(cfg)
    model.load_weights(weights)
    from bayes_od_rc_amd.anchor_generator import FpnAnchorGenerator
    from test_gpu_train_from_boxes import _gt_from_anchors
    small = FpnAnchorGenerator(ANCHOR_CFG).generate_all((64, 64, 3)).astype(np.float32)
    trainer = Engine(make_config((64, 64), batch=1, mc_samples=1, training=True))
    trainer.load_weights(weights)
    trainer.set_anchors(small)
    gt = _gt_from_anchors(small, 0)
    out = trainer.train_step_boxes(synthetic.make_frames(1, 64, 64, seed=5), [gt[0]], [gt[1]], 0.5, 0.4, l2_rate=1e-6, apply_update=False)
    trainer.close()
    print("regularization_loss", model.regularization_loss(), out["regularization_loss"])
    assert out["regularization_loss"] > 0
    assert abs(model.regularization_loss() - out["regularization_loss"]) <= 1e-5 * out["regularization_loss"]


def test_refusals(problem):
    from bayes_od_rc_amd.engine import Engine, make_config
    p = problem
    boxes, classes = p.gt_boxes[:1], p.gt_classes[:1]
    eng = Engine(make_config((64, 64), batch=1, mc_samples=1, training=True))
    with pytest.raises(ValueError, match="training handle"):
        eng.validation_losses_boxes(boxes, classes)
    eng.close()
    many = Engine(make_config(HW, batch=1, mc_samples=2, nms_config=NMS_CFG))
    with pytest.raises(ValueError, match="one deterministic sample"):
        many.validate_boxes(np.zeros((1,) + HW + (3,), np.float32), boxes, classes)
    with pytest.raises(ValueError, match="one deterministic sample"):
        many.validation_losses_boxes(boxes, classes)
    many.close()
    with pytest.raises(ValueError, match="4 or 8"):                    # a class count the loss kernels do not support
        Engine(make_config(HW, batch=1, mc_samples=1, num_classes=5, anchors_per_location=8))
    eng = _engine(1, has_covar_head=False)
    with pytest.raises(ValueError, match="covariance head"):
        eng.validation_losses_boxes(boxes, classes, reg_kind=2)
    with pytest.raises(ValueError, match="covariance head"):
        eng.validate_boxes(np.zeros((1,) + HW + (3,), np.float32), boxes, classes, reg_kind=3)
    eng.close()
    eng = _engine(1)
    with pytest.raises(ValueError, match="ground-truth rows"):
        eng.validation_losses_boxes([np.zeros((0, 4), np.float32)], [np.zeros((0, 8), np.float32)])
    with pytest.raises(RuntimeError, match="bod_set_anchors"):
        eng.validation_losses_boxes(boxes, classes)
    eng.set_anchors(p.anchors)
    with pytest.raises(RuntimeError, match="has not run"):
        eng.validation_losses_boxes(boxes, classes)
    with pytest.raises(RuntimeError, match="weights not finalized"):
        eng.validate_boxes(np.zeros((1,) + HW + (3,), np.float32), boxes, classes)
    _set(eng, p, [0])
    with pytest.raises(RuntimeError, match="bod_nms has not run"):
        eng.validation_detections_batch()
    assert np.isfinite(eng.validation_losses_boxes(boxes, classes)).all()          # ... and the handle still works
    eng.close()


def _config(tmp_path, monkeypatch, edit=None, name="retinanet_bdd_covar"):
    """The packaged yaml, optionally edited and written under tmp_path (the file name must equal checkpoint_name)."""
    import yaml
    from bayes_od_rc_amd import config_utils, run_validation
    monkeypatch.setenv("BAYESOD_DATA_DIR", str(tmp_path / "data"))
    here = os.path.dirname(os.path.abspath(run_validation.__file__))
    cfg = config_utils.load_yaml(os.path.join(here, "configs", name + ".yaml"))
    if edit:
        edit(cfg)
    ypath = tmp_path / (name + ".yaml")
    ypath.write_text(yaml.safe_dump(cfg))
    return str(ypath)


def _checkpoint(tmp_path, num_classes_with_bknd, step=1, name="retinanet_bdd_covar"):
    from bayes_od_rc_amd import synthetic
    from bayes_od_rc_amd.model import RetinaNetModel
    ckpt_dir = tmp_path / "data" / "outputs" / name / "checkpoints"
    ckpt_dir.mkdir(parents=True)
    path = str(ckpt_dir / ("ckpt-%d.npz" % step))
    RetinaNetModel.save_weights_npz(synthetic.make_weights(num_classes_with_bknd, 9, cls_fg_bias=FG_BIAS), path)
    return path


def test_run_validation_streams_a_bdd_tree(tmp_path, monkeypatch):
    """--dataset --batch 3 over 4 frames of a BDD-shaped tree (a tail batch of 1): no dense targets on the host, never more than
    one batch of sample dicts alive, predictions in dataset order, and the losses of the dense per-frame route."""
    from PIL import Image
    from bayes_od_rc_amd import box_utils, config_utils, datasets, run_validation
    root = tmp_path / "bdd100k"
    (root / "images" / "100k" / "val").mkdir(parents=True)
    (root / "labels").mkdir()
    rng = np.random.default_rng(6)
    names, labels = ["%04d.png" % i for i in range(4)], []
    for i, name in enumerate(names):
        Image.fromarray(rng.integers(0, 256, size=(128, 128, 3), dtype=np.uint8)).save(str(root / "images" / "100k" / "val" / name))
        if i == 2:
            labels.append({"name": name, "category": "traffic light", "bbox": [5.0, 5.0, 30.0, 40.0]})       # no trained category
        else:
            labels.append({"name": name, "category": "car", "bbox": [20.0, 30.0, 90.0, 80.0]})
            labels.append({"name": name, "category": "person", "bbox": [60.0 + i, 10.0, 100.0, 70.0]})
    (root / "labels" / "val.json").write_text(json.dumps(labels))

    def edit(cfg):
        cfg["dataset_config"]["bdd"]["paths_config"]["dataset_dir"] = str(root)
    ypath = _config(tmp_path, monkeypatch, edit)
    ckpt = _checkpoint(tmp_path, 8)

    # the reference values first: dense samples through the per-frame route, into a directory of their own
    class Args(object):
        data_split, yaml_path = "val", ypath
    config = config_utils.setup(config_utils.load_yaml(ypath), Args())
    handler = datasets.build_dataset(config["dataset_config"], "val")
    dense = list(handler.create_dataset())
    assert all("anchors_class_targets" in s for s in dense) and list(handler.sample_ids) == names
    categories = handler.training_data_config["categories"]
    ref = run_validation.validate_checkpoint(config, ckpt, dense, names, str(tmp_path / "dense_predictions"), categories)
    del dense, handler

    class Sample(dict):                   # (a dict that can be weakly referenced)
        pass
    refs, peak, placeholders = [], [], []

    def alive():
        gc.collect()
        return sum(r() is not None for r in refs)
    real_create = datasets.create_sample_dict

    def counting_create(*args, **kwargs):
        assert kwargs.get("dense_targets") is False
        peak.append(alive() + 1)                                       # sample dicts alive once this one exists
        sample = Sample(real_create(*args, **kwargs))
        assert "anchors_class_targets" not in sample and "positive_anchors_mask" not in sample
        refs.append(weakref.ref(sample))
        placeholders.append(np.array_equal(sample["boxes_2d_gt"], [[0.0, 0.0, 1.0, 1.0]]))
        return sample

    def no_iou(*a, **k):
        raise AssertionError("the dataset route must not build dense targets on the host")
    monkeypatch.setattr(datasets, "create_sample_dict", counting_create)
    monkeypatch.setattr(box_utils, "bbox_iou_vuvu", no_iou)
    real_batch, seen = run_validation.validate_batch, []

    def watched_batch(model, config, batch):
        seen.append((len(refs), alive(), len(batch)))
        return real_batch(model, config, batch)
    monkeypatch.setattr(run_validation, "validate_batch", watched_batch)
    res = run_validation.main(["--gpu_device", "0", "--yaml_path", ypath, "--data_split", "val", "--dataset", "--batch", "3"])
    assert len(res) == 1 and res[0]["ckpt_id"] == 1 and res[0]["num_frames"] == 4
    r = res[0]
    # the full batch starts with three samples read and alive, the tail batch with the fourth alone
    assert seen == [(3, 3, 3), (4, 1, 1)], seen
    assert max(peak) <= 3 and len(peak) == 4, peak
    assert placeholders == [False, False, True, False]
    pred_root = os.path.join(str(tmp_path / "data"), "outputs", "retinanet_bdd_covar", "predictions")
    with open(os.path.join(pred_root, "validation", "1", "data", "predictions.json")) as fp:
        records = json.load(fp)
    print("detections", r["num_detections"], "losses", r["mean_total_loss"], r["mean_losses"], "dense", ref["mean_total_loss"], ref["mean_losses"])
    assert len(records) == r["num_detections"] and r["num_detections"] >= 1
    order = [names.index(rec["name"]) for rec in records]
    assert order == sorted(order)                                       # dataset order, whatever the bucketing did
    assert list(run_validation.get_evaluated_ckpts(pred_root)) == [1]
    assert set(r["mean_losses"]) == {"cls_loss", "reg_loss", "covariance_loss", "regularization_loss"}
    assert np.isfinite(r["mean_total_loss"]) and all(np.isfinite(v) for v in r["mean_losses"].values())
    assert r["mean_losses"]["regularization_loss"] > 0
    got = r["mean_total_loss"] - r["mean_losses"]["regularization_loss"]
    assert abs(got - ref["mean_total_loss"]) <= 1e-5 * abs(ref["mean_total_loss"]) + 1e-7, (got, ref["mean_total_loss"])
    assert r["num_detections"] == ref["num_detections"]


def test_run_validation_on_a_kitti_tree(tmp_path, monkeypatch):
    """--dataset on KITTI (this raised before: the handler leaves the pixels to the device): two source sizes interleaved, so
    --batch 2 forms full batches by bucketing and flushes a tail per size; one text file per frame."""
    from PIL import Image
    from bayes_od_rc_amd import run_validation
    root = tmp_path / "object"
    (root / "training" / "image_2").mkdir(parents=True)
    (root / "training" / "label_2").mkdir()
    ids = ["%06d" % i for i in range(6)]
    (root / "val.txt").write_text("\n".join(ids) + "\n")
    rng = np.random.default_rng(5)
    for i, sid in enumerate(ids):
        hw = (94, 310) if i % 2 == 0 else (92, 306)
        Image.fromarray(rng.integers(0, 256, size=hw + (3,), dtype=np.uint8)).save(str(root / "training" / "image_2" / (sid + ".png")))
        (root / "training" / "label_2" / (sid + ".txt")).write_text(
            "Car 0.00 0 -1.57 100.00 20.00 200.00 80.00 1.5 1.6 3.9 1.0 1.5 10.0 -1.5\n"
            "Pedestrian 0.00 0 0.10 30.00 10.00 60.00 70.00 1.8 0.6 0.8 -3.0 1.5 12.0 0.1\n")

    def edit(cfg):
        cfg["dataset_config"]["dataset"] = "kitti"        # config_utils.setup then derives num_classes = 3 from KITTI's categories
        cfg["dataset_config"]["kitti"]["paths_config"]["dataset_dir"] = str(root)
        cfg["dataset_config"]["kitti"]["resize_shape"] = [128, 416]
    ypath = _config(tmp_path, monkeypatch, edit)
    _checkpoint(tmp_path, 4)
    real_batch, seen = run_validation.validate_batch, []

    def watched_batch(model, config, batch):
        seen.append(tuple(int(v) for v in batch[0]["im_size"][:2]) + (len(batch),))
        return real_batch(model, config, batch)
    monkeypatch.setattr(run_validation, "validate_batch", watched_batch)
    res = run_validation.main(["--gpu_device", "0", "--yaml_path", ypath, "--data_split", "val", "--dataset", "--batch", "2"])
    assert len(res) == 1 and res[0]["num_frames"] == 6 and res[0]["predictions"] is None
    assert seen == [(94, 310, 2), (92, 306, 2), (92, 306, 1), (94, 310, 1)], seen
    r = res[0]
    print("kitti", r["mean_total_loss"], r["mean_losses"], r["num_detections"])
    assert np.isfinite(r["mean_total_loss"]) and all(np.isfinite(v) for v in r["mean_losses"].values())
    assert set(r["mean_losses"]) == {"cls_loss", "reg_loss", "covariance_loss", "regularization_loss"}
    out_dir = os.path.join(str(tmp_path / "data"), "outputs", "retinanet_bdd_covar", "predictions", "validation", "1", "data")
    assert sorted(os.listdir(out_dir)) == [sid + ".txt" for sid in ids]
