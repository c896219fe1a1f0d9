"""GPU: --device_png of run_inference, run_validation and run_training on a four-frame KITTI tree of PNG files with
two source sizes: the PNG upload route is taken, and the results equal the run without the flag (the PIL route)."""
import os
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LABELS = ("Car 0.00 0 -1.57 100.00 20.00 200.00 80.00 1.5 1.6 3.9 1.0 1.5 10.0 -1.5\n"
          "Pedestrian 0.00 0 0.10 30.00 10.00 60.00 70.00 1.8 0.6 0.8 -3.0 1.5 12.0 0.1\n")


def _tree(tmp_path, split):
    """Frames of sizes A, B, A, B; the last one a gray file (colour type 0), the others RGB."""
    from PIL import Image
    root = tmp_path / "object"
    (root / "training" / "image_2").mkdir(parents=True)
    (root / "training" / "label_2").mkdir()
    ids = ["%06d" % i for i in range(4)]
    (root / (split + ".txt")).write_text("\n".join(ids) + "\n")
    rng = np.random.default_rng(5)
    for i, sid in enumerate(ids):
        hw = (94, 310) if i % 2 == 0 else (92, 306)
        frame = rng.integers(0, 256, size=hw + (3,), dtype=np.uint8)
        Image.fromarray(frame[:, :, 0] if i == 3 else frame).save(str(root / "training" / "image_2" / (sid + ".png")))
        (root / "training" / "label_2" / (sid + ".txt")).write_text(LABELS)
    return root, ids


def _count_png_uploads(monkeypatch):
    from bayes_od_rc_amd.engine import Engine
    calls, real = [], Engine.upload_frames_png
    monkeypatch.setattr(Engine, "upload_frames_png", lambda self, files, *a, **k: (calls.append((len(files), k.get("aug") is not None)),
                                                                                  real(self, files, *a, **k))[1])
    return calls


def _kitti(root):
    def edit(cfg):
        cfg["dataset_config"]["dataset"] = "kitti"        # config_utils.setup then derives num_classes = 3 from KITTI's categories
        cfg["dataset_config"]["kitti"]["paths_config"]["dataset_dir"] = str(root)
        cfg["dataset_config"]["kitti"]["resize_shape"] = [128, 416]
    return edit


def test_run_inference_device_png_writes_the_same_files(tmp_path, monkeypatch):
    from bayes_od_rc_amd import run_inference, synthetic
    from bayes_od_rc_amd.model import RetinaNetModel
    from test_gpu_mixed_sizes import _yaml
    root, ids = _tree(tmp_path, "test")
    weights = str(tmp_path / "weights.npz")                  # (the default synthetic class bias, -4.6, detects nothing on these frames)
    RetinaNetModel.save_weights_npz(synthetic.make_weights(8, 9, cls_fg_bias=-1.0), weights)

    def edit(cfg):
        cfg["testing_config"]["test_dataset"] = "kitti"
    ypath = _yaml(tmp_path, root, edit)
    args = ["--gpu_device", "0", "--yaml_path", ypath, "--data_split", "test", "--dataset", "--batch", "2", "--weights", weights]
    calls = _count_png_uploads(monkeypatch)
    monkeypatch.setenv("BAYESOD_DATA_DIR", str(tmp_path / "default"))
    ref = run_inference.main(args)
    assert calls == []
    monkeypatch.setenv("BAYESOD_DATA_DIR", str(tmp_path / "png"))
    out = run_inference.main(args + ["--device_png"])
    assert calls == [(2, False), (2, False)]                 # both batches hold frames of two sizes and are decoded on the device
    monkeypatch.setenv("BAYESOD_DATA_DIR", str(tmp_path / "both"))
    both = run_inference.main(args + ["--device_png", "--device_jpeg"])
    assert calls == [(2, False)] * 4 and len({ref, out, both}) == 3
    listing = sorted(os.path.relpath(os.path.join(d, f), ref) for d, _, fs in os.walk(ref) for f in fs)
    assert len(listing) >= 4 * 4
    for other in (out, both):
        assert listing == sorted(os.path.relpath(os.path.join(d, f), other) for d, _, fs in os.walk(other) for f in fs)
        for rel in listing:
            with open(os.path.join(ref, rel), "rb") as fa, open(os.path.join(other, rel), "rb") as fb:
                assert fa.read() == fb.read(), rel
    total = sum(np.load(os.path.join(out, "mean", sid + ".npy")).shape[0] for sid in ids)
    print("detections over the four frames:", total)
    assert total >= 4
    with pytest.raises(SystemExit):
        run_inference.main(["--gpu_device", "0", "--data_split", "test", "--synthetic", "2", "--device_png"])


def test_run_validation_device_png_equals_the_pil_route(tmp_path, monkeypatch):
    from bayes_od_rc_amd import run_validation
    from test_gpu_validation_boxes import _checkpoint, _config
    root, _ = _tree(tmp_path, "val")
    calls = _count_png_uploads(monkeypatch)
    results = {}
    # the PIL route with the batches --device_png forms is --mixed_sizes (the default route buckets by size: the same frames in
    # another order, and a float64 mean of per-frame losses depends on the order in its last digit).  A data directory each: a
    # checkpoint is validated once
    for route, flag in (("default", ["--mixed_sizes"]), ("png", ["--device_png"]), ("bucketed", [])):
        (tmp_path / route).mkdir()
        ypath = _config(tmp_path / route, monkeypatch, _kitti(root))
        _checkpoint(tmp_path / route, 4)
        results[route] = run_validation.main(["--gpu_device", "0", "--yaml_path", ypath, "--data_split", "val", "--dataset", "--batch", "2"] + flag)
        assert calls == ([] if route == "default" else [(2, False), (2, False)])      # (none more in the last run: no flag)
    ref, got = results["default"], results["png"]
    assert len(ref) == len(got) == 1 and got[0]["num_frames"] == 4
    print("losses", got[0]["mean_total_loss"], got[0]["mean_losses"], "detections", got[0]["num_detections"])
    assert got[0]["mean_total_loss"] == ref[0]["mean_total_loss"] and got[0]["mean_losses"] == ref[0]["mean_losses"]
    assert got[0]["num_detections"] == ref[0]["num_detections"]
    # ... and the run with neither flag: the same per-frame float64 losses averaged in another order, so equal to a few ulps of the
    # mean (4 terms: at most 3 roundings of 2^-53 relative each in either order; 1e-12 is 1500 times that,
    # room for per-frame terms that partly cancel)
    plain = results["bucketed"]
    assert plain[0]["num_frames"] == 4 and plain[0]["num_detections"] == got[0]["num_detections"]
    assert abs(plain[0]["mean_total_loss"] - got[0]["mean_total_loss"]) <= 1e-12 * abs(plain[0]["mean_total_loss"])
    for key, value in plain[0]["mean_losses"].items():
        assert abs(value - got[0]["mean_losses"][key]) <= 1e-12 * abs(value), key
    with pytest.raises(SystemExit):
        run_validation.main(["--gpu_device", "0", "--yaml_path", ypath, "--device_png"])


def test_run_training_device_png_with_augment_equals_the_pil_route(tmp_path, monkeypatch):
    from bayes_od_rc_amd import run_training
    from test_gpu_validation_boxes import _config
    root, _ = _tree(tmp_path, "train")
    calls = _count_png_uploads(monkeypatch)
    histories = []
    for i, extra in enumerate((["--augment"], ["--augment", "--device_png"])):
        (tmp_path / ("run%d" % i)).mkdir()                       # a data directory each: no run resumes another's checkpoint
        ypath = _config(tmp_path / ("run%d" % i), monkeypatch, _kitti(root))
        random.seed(11)                                          # the handler shuffles the training split
        np.random.seed(11)
        history, _ = run_training.main(["--gpu_device", "0", "--yaml_path", ypath, "--data_split", "train", "--dataset", "--steps", "1"] + extra)
        assert len(history) == 1 and np.isfinite(history).all(), (extra, history)
        histories.append(list(history))
    print("loss histories", histories)
    assert calls == [(3, True)]
    # the step sees the same bytes and the same weights.  Its total is cls + reg + covariance + L2; the L2 term is summed with float
    # atomics and is reproducible to 1e-5 of itself only, in any route (tests/test_gpu_mixed_sizes.py), and it is at
    # most the total: that is the bound
    assert abs(histories[1][0] - histories[0][0]) <= 1e-5 * histories[0][0], histories
    with pytest.raises(SystemExit):
        run_training.main(["--gpu_device", "0", "--yaml_path", ypath, "--device_png"])
