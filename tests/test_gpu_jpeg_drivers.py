"""GPU: --device_jpeg of run_validation and run_training on BDD-layout trees of small JPEG files: the JPEG upload
route is taken, and the results equal the run without the flag."""
import json
import os
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _tree(tmp_path, split, names):
    from PIL import Image
    root = tmp_path / "bdd100k"
    (root / "images" / "100k" / split).mkdir(parents=True)
    (root / "labels").mkdir()
    rng = np.random.default_rng(6)
    labels = []
    for i, name in enumerate(names):
        im = Image.fromarray(rng.integers(0, 256, size=(128, 128, 3), dtype=np.uint8))
        path = str(root / "images" / "100k" / split / name)
        if name.endswith(".jpg"):
            im.save(path, quality=85, subsampling=("4:2:0", "4:2:2", "4:4:4")[i % 3])
        else:
            im.save(path)
        labels.append({"name": name, "category": "car", "bbox": [20.0, 30.0, 90.0, 80.0]})
        labels.append({"name": name, "category": "person", "bbox": [60.0 + i, 10.0, 100.0, 70.0]})
    (root / "labels" / (split + ".json")).write_text(json.dumps(labels))
    return root


def _count_jpeg_uploads(monkeypatch):
    from bayes_od_rc_amd.engine import Engine
    calls, real = [], Engine.upload_frames_jpeg
    monkeypatch.setattr(Engine, "upload_frames_jpeg", lambda self, files, *a, **k: (calls.append((len(files), k.get("aug") is not None)),
                                                                                   real(self, files, *a, **k))[1])
    return calls


def test_run_validation_device_jpeg_equals_the_default_route(tmp_path, monkeypatch):
    from bayes_od_rc_amd import run_validation
    from test_gpu_validation_boxes import _checkpoint, _config
    root = _tree(tmp_path, "val", ["a.jpg", "b.jpg", "c.jpg", "d.png"])

    def edit(cfg):
        cfg["dataset_config"]["bdd"]["paths_config"]["dataset_dir"] = str(root)
    calls = _count_jpeg_uploads(monkeypatch)
    results = {}
    for route, flag in (("default", []), ("jpeg", ["--device_jpeg"])):           # a data directory each: a checkpoint is validated once
        (tmp_path / route).mkdir()
        ypath = _config(tmp_path / route, monkeypatch, edit)
        _checkpoint(tmp_path / route, 8)
        results[route] = run_validation.main(["--gpu_device", "0", "--yaml_path", ypath, "--data_split", "val", "--dataset", "--batch", "2"] + flag)
        assert calls == ([] if route == "default" else [(2, False)])     # (a, b) on the device; (c, d.png) by PIL
    ref, got = results["default"], results["jpeg"]
    assert len(ref) == len(got) == 1 and got[0]["num_frames"] == 4
    print("losses", got[0]["mean_total_loss"], got[0]["mean_losses"], "detections", got[0]["num_detections"])
    assert got[0]["mean_total_loss"] == ref[0]["mean_total_loss"] and got[0]["mean_losses"] == ref[0]["mean_losses"]
    assert got[0]["num_detections"] == ref[0]["num_detections"]
    with pytest.raises(SystemExit):
        run_validation.main(["--gpu_device", "0", "--yaml_path", ypath, "--device_jpeg"])


def test_run_training_device_jpeg_equals_the_default_route(tmp_path, monkeypatch):
    from bayes_od_rc_amd import run_training
    from test_gpu_validation_boxes import _config
    root = _tree(tmp_path, "train", ["a.jpg", "b.jpg", "c.jpg", "d.jpg"])

    def edit(cfg):
        cfg["dataset_config"]["bdd"]["paths_config"]["dataset_dir"] = str(root)
    calls = _count_jpeg_uploads(monkeypatch)
    histories = []
    for i, extra in enumerate(([], ["--device_jpeg"], ["--augment"], ["--augment", "--device_jpeg"])):
        (tmp_path / ("run%d" % i)).mkdir()                       # a data directory each: no run resumes another's checkpoint
        ypath = _config(tmp_path / ("run%d" % i), monkeypatch, edit)
        random.seed(11)                                          # the handler shuffles the training split
        np.random.seed(11)
        history, _ = run_training.main(["--gpu_device", "0", "--yaml_path", ypath, "--data_split", "train", "--dataset", "--steps", "2"] + extra)
        assert len(history) == 2 and np.isfinite(history).all(), (extra, history)
        histories.append(list(history))
    print("loss histories", histories)
    assert calls == [(3, False), (3, False), (3, True), (3, True)]
    # the first step sees the same bytes and the same weights.  Its total is cls + reg + covariance + L2; the L2 term is summed with
    # float atomics and is reproducible to 1e-5 of itself only, in any route (tests/test_gpu_mixed_sizes.py), and it
    # is at most the total: that is the bound
    for with_flag, without in ((1, 0), (3, 2)):
        assert abs(histories[with_flag][0] - histories[without][0]) <= 1e-5 * histories[without][0], (histories[with_flag], histories[without])
    with pytest.raises(SystemExit):
        run_training.main(["--gpu_device", "0", "--yaml_path", ypath, "--device_jpeg"])
