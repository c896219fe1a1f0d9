"""GPU: the training step from ground-truth boxes (bod_train_step_boxes): the step uses the targets the device assigned, it is
the same step as the dense route, Trainer.train_single_step takes GT-only samples, and run_training --dataset streams a KITTI
and a BDD-shaped tree."""
import gc
import json
import os
import weakref

import numpy as np
import pytest

from conftest import ANCHOR_CFG

pytestmark = pytest.mark.gpu

LOSS_KEYS = ("total_loss", "cls_loss", "reg_loss", "covariance_loss", "regularization_loss", "grad_norm")


def _gt_from_anchors(anchors, seed, num_classes=8):
    """Four anchors with h <= 64 picked at random, sizes x 1.1, centres + 2 px, turned to corners."""
    from bayes_od_rc_amd import box_utils
    rng = np.random.default_rng(seed)
    pick = anchors[rng.choice(np.nonzero(anchors[:, 2] <= 64)[0], 4, replace=False)].copy()
    pick[:, 2:] *= np.float32(1.1)
    pick[:, :2] += np.float32(2.0)
    boxes = box_utils.vuhw_to_vuvu_np(pick).astype(np.float32)
    classes = np.eye(num_classes, dtype=np.float32)[rng.integers(0, num_classes - 1, 4)]
    return boxes, classes


def _problem(hw=(64, 64), batch=2, precision="bf16"):
    from bayes_od_rc_amd import synthetic
    from bayes_od_rc_amd.anchor_generator import FpnAnchorGenerator
    from bayes_od_rc_amd.engine import Engine, make_config
    from bayes_od_rc_amd.sample_builder import create_sample_dict
    weights = synthetic.make_weights(cls_fg_bias=-2.0)
    anchors = FpnAnchorGenerator(ANCHOR_CFG).generate_all(hw + (3,)).astype(np.float32)
    frames = synthetic.make_frames(batch, hw[0], hw[1], seed=5)
    gt = [_gt_from_anchors(anchors, seed) for seed in range(batch)]
    dense = [create_sample_dict(frames[b], ANCHOR_CFG, gt[b][0], gt[b][1]) for b in range(batch)]
    for s in dense:
        assert s["positive_anchors_mask"].sum() >= 50                  # (169-196 of 774 for seeds 0-2 on the host)
    eng = Engine(make_config(hw, batch=batch, mc_samples=1, training=True, precision=precision))
    eng.load_weights(weights)
    eng.set_anchors(anchors)
    return eng, weights, anchors, frames, gt, dense


def test_the_step_uses_the_assigned_targets():
    from bayes_od_rc_amd.engine import anchor_targets
    eng, _, anchors, frames, gt, dense = _problem()
    boxes, classes = [g[0] for g in gt], [g[1] for g in gt]
    out = eng.train_step_boxes(frames, boxes, classes, 0.5, 0.4, seed=3, first_image_id=10, apply_update=False)
    assert all(np.isfinite(out[k]) for k in LOSS_KEYS), out
    used = eng.train_targets()
    want = anchor_targets(anchors, boxes, classes, 0.5, 0.4)
    for u, w in zip(used, want):
        assert u.dtype == w.dtype and np.array_equal(u, w)
    assert np.array_equal(used[2], np.stack([s["positive_anchors_mask"] for s in dense]))
    # ... and bod_train_get_targets reads whatever the last step used: the dense route's copies too
    cls_t = np.stack([s["anchors_class_targets"] for s in dense])
    box_t = np.stack([s["anchors_box_targets"] for s in dense])
    pos = np.stack([s["positive_anchors_mask"] for s in dense])
    neg = np.stack([s["negative_anchors_mask"] for s in dense])
    eng.train_step(frames, cls_t, box_t, pos, neg, seed=3, first_image_id=10, apply_update=False)
    back = eng.train_targets()
    assert np.array_equal(back[0], cls_t) and np.array_equal(back[1], box_t) and np.array_equal(back[2], pos) and np.array_equal(back[3], neg)
    with pytest.raises(ValueError, match="ground-truth rows"):
        eng.train_step_boxes(frames, [boxes[0], np.zeros((0, 4), np.float32)], [classes[0], np.zeros((0, 8), np.float32)], 0.5, 0.4)
    eng.close()


def test_same_step_as_the_dense_route_on_the_fp32_handle():
    """train_step_boxes against train_step fed with the host generator's dense targets: loss terms and gradient norm to
    1e-5 |ref| + 1e-7, every gradient tensor to 1e-4 max|g| -- the bounds test_gpu_train_step.py holds this handle to against
    float64 autograd (bitwise equality is not available: the step's gradient adds are atomic)."""
    eng, weights, anchors, frames, gt, dense = _problem(precision="fp32")

    def grads():
        out = {}
        for layer, fields in weights.items():
            for kind in ("kernel", "bias", "gamma", "beta"):
                a = fields.get(kind)
                if a is None:
                    continue
                try:
                    out[layer + "/" + kind] = eng.train_get(layer, kind, np.asarray(a).shape, what="grad").astype(np.float64)
                except ValueError:
                    pass                                  # not a variable of the model (RegHeader's never-called conv_4)
        return out
    got = eng.train_step_boxes(frames, [g[0] for g in gt], [g[1] for g in gt], 0.5, 0.4, seed=3, first_image_id=10, apply_update=False)
    g_boxes = grads()
    ref = eng.train_step(frames, np.stack([s["anchors_class_targets"] for s in dense]), np.stack([s["anchors_box_targets"] for s in dense]),
                         np.stack([s["positive_anchors_mask"] for s in dense]), np.stack([s["negative_anchors_mask"] for s in dense]),
                         seed=3, first_image_id=10, apply_update=False)
    g_dense = grads()
    for k in LOSS_KEYS:
        print(k, got[k], ref[k])
        assert abs(got[k] - ref[k]) <= 1e-5 * abs(ref[k]) + 1e-7, (k, got[k], ref[k])
    assert ref["reg_loss"] > 0 and ref["grad_norm"] > 0
    checked, worst = 0, (0.0, None)
    for name, g in g_dense.items():
        scale = np.abs(g).max()
        if scale < 1e-9 * ref["grad_norm"]:
            assert np.abs(g_boxes[name]).max() <= 1e-7 * ref["grad_norm"], name
            continue
        err = float(np.abs(g_boxes[name] - g).max() / scale)
        worst = max(worst, (err, name))
        assert err <= 1e-4, (name, err)
        checked += 1
    assert checked > 250, checked
    print("worst gradient difference / max|g|: %.2e (%s), %d tensors" % (worst[0], worst[1], checked))
    eng.close()


def _config(tmp_path, monkeypatch, edit=None, name="retinanet_bdd_covar"):
    """The packaged yaml, optionally edited and written under tmp_path (the file name must equal checkpoint_name)."""
    import yaml
    from bayes_od_rc_amd import config_utils, run_training
    monkeypatch.setenv("BAYESOD_DATA_DIR", str(tmp_path / "data"))
    here = os.path.dirname(os.path.abspath(run_training.__file__))
    cfg = config_utils.load_yaml(os.path.join(here, "configs", name + ".yaml"))
    if edit:
        edit(cfg)
    ypath = tmp_path / (name + ".yaml")
    ypath.write_text(yaml.safe_dump(cfg))
    return str(ypath)


@pytest.mark.parametrize("graph", ["0", "1"])
def test_trainer_takes_ground_truth_only_samples(graph, tmp_path, monkeypatch):
    from bayes_od_rc_amd import config_utils, synthetic
    from bayes_od_rc_amd.run_training import Trainer
    from bayes_od_rc_amd.sample_builder import create_sample_dict
    monkeypatch.setenv("BOD_TRAIN_GRAPH", graph)
    ypath = _config(tmp_path, monkeypatch)

    class Args(object):
        data_split, yaml_path = "train", ypath
    config = config_utils.setup(config_utils.load_yaml(ypath), Args())
    hw, mb = (64, 64), int(config["training_config"]["minibatch_size"])
    anchor_cfg = config["dataset_config"]["anchor_generator"]
    frames = synthetic.make_frames(mb, hw[0], hw[1], seed=5)
    samples = []
    for b in range(mb):
        sample = create_sample_dict(frames[b], anchor_cfg, is_testing=True)
        boxes, classes = _gt_from_anchors(sample["anchors"], b)
        samples.append(create_sample_dict(frames[b], anchor_cfg, boxes, classes, dense_targets=False))
        assert "anchors_class_targets" not in samples[-1] and "boxes_2d_gt" in samples[-1]
    trainer = Trainer(config, hw, synthetic.make_weights(8, 9), device=0, seed=0)
    losses = []
    for _ in range(8):
        total, loss_dict = trainer.train_single_step(samples, 1e-3)
        assert set(loss_dict) == {"cls_loss", "reg_loss", "regularization_loss", "covariance_loss"}
        assert np.isfinite(total) and all(np.isfinite(v) for v in loss_dict.values()), (total, loss_dict)
        losses.append(total)
    assert trainer.step == 8 and losses[-1] < losses[0], losses
    # the thresholds came from the config's anchor_generator block
    from bayes_od_rc_amd.engine import anchor_targets
    want = anchor_targets(samples[0]["anchors"], [s["boxes_2d_gt"] for s in samples], [s["boxes_class_gt"] for s in samples],
                          anchor_cfg["min_positive_iou"], anchor_cfg["max_negative_iou"])
    for u, w in zip(trainer.engine.train_targets(), want):
        assert np.array_equal(u, w)
    trainer.engine.close()


def test_run_training_on_a_kitti_tree(tmp_path, monkeypatch):
    """--dataset on KITTI: frames of two source sizes, interleaved, so the yaml's minibatch of 3 only forms by bucketing; the
    frames are resized on the device and the targets assigned there (this raised ValueError before)."""
    from PIL import Image
    from bayes_od_rc_amd import run_training
    root = tmp_path / "object"
    (root / "training" / "image_2").mkdir(parents=True)
    (root / "training" / "label_2").mkdir()
    ids = ["%06d" % i for i in range(6)]
    (root / "train.txt").write_text("\n".join(ids) + "\n")
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
    history, ckpt_dir = run_training.main(["--gpu_device", "0", "--yaml_path", ypath, "--data_split", "train", "--dataset", "--steps", "4"])
    assert len(history) == 4 and np.isfinite(history).all(), history
    assert os.path.exists(os.path.join(ckpt_dir, "ckpt-4.npz"))


def test_run_training_streams_a_bdd_tree(tmp_path, monkeypatch):
    """--dataset on a BDD-shaped tree: sample dicts are made one minibatch at a time, never with dense targets, and one frame
    has no box of a trained category (the placeholder row)."""
    from PIL import Image
    from bayes_od_rc_amd import box_utils, datasets, run_training
    root = tmp_path / "bdd100k"
    (root / "images" / "100k" / "train").mkdir(parents=True)
    (root / "labels").mkdir()
    rng = np.random.default_rng(6)
    names, labels = ["%04d.png" % i for i in range(4)], []
    for i, name in enumerate(names):
        Image.fromarray(rng.integers(0, 256, size=(128, 128, 3), dtype=np.uint8)).save(str(root / "images" / "100k" / "train" / name))
        if i == 2:
            labels.append({"name": name, "category": "traffic light", "bbox": [5.0, 5.0, 30.0, 40.0]})
        else:
            labels.append({"name": name, "category": "car", "bbox": [20.0, 30.0, 90.0, 80.0]})
            labels.append({"name": name, "category": "person", "bbox": [60.0 + i, 10.0, 100.0, 70.0]})
    (root / "labels" / "train.json").write_text(json.dumps(labels))

    def edit(cfg):
        cfg["dataset_config"]["bdd"]["paths_config"]["dataset_dir"] = str(root)
    ypath = _config(tmp_path, monkeypatch, edit)

    class Sample(dict):                   # (a dict that can be weakly referenced)
        pass
    refs, calls, placeholders, peak = [], [], [], []

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
        calls.append(1)
        placeholders.append(np.array_equal(sample["boxes_2d_gt"], [[0.0, 0.0, 1.0, 1.0]]))
        return sample

    def no_iou(*a, **k):
        raise AssertionError("the dataset route must not build dense targets on the host")
    monkeypatch.setattr(datasets, "create_sample_dict", counting_create)
    monkeypatch.setattr(box_utils, "bbox_iou_vuvu", no_iou)
    real_step, seen = run_training.Trainer.train_single_step, []

    def watched_step(self, sample_dicts, learning_rate):
        seen.append((len(calls), alive(), len(sample_dicts)))
        return real_step(self, sample_dicts, learning_rate)
    monkeypatch.setattr(run_training.Trainer, "train_single_step", watched_step)
    history, ckpt_dir = run_training.main(["--gpu_device", "0", "--yaml_path", ypath, "--data_split", "train", "--dataset", "--steps", "3"])
    assert len(history) == 3 and np.isfinite(history).all(), history
    # step k starts with exactly (k + 1) minibatches read from the handler and one minibatch of sample dicts alive
    assert seen == [(3, 3, 3), (6, 3, 3), (9, 3, 3)], seen
    assert max(peak) <= 3, peak                                        # never more than one minibatch of sample dicts
    assert sum(placeholders) >= 2                                      # the frame without a trained category came by (4 frames, 9 reads)
    assert os.path.exists(os.path.join(ckpt_dir, "ckpt-3.npz"))
