"""GPU: the drivers of the rendering stage end to end on tiny trees: ``python -m bayes_od_rc_amd.show_predictions``
writes PNGs that decode to exactly ``render.render_frames``' bytes, and ``run_inference --render`` writes one file per frame and view,
from synthetic frames and from a BDD-layout dataset whose JPEG files travel to the device as bytes."""
import json
import os

import numpy as np
import pytest

import conftest  # noqa: F401

pytestmark = pytest.mark.gpu

CATEGORIES = ["car", "truck", "bus", "person", "rider", "bike", "motor"]


def _tree(tmp_path):
    """Three frames of two sizes: a prediction tree (with one covariance part), the images as PNG files, BDD labels."""
    from PIL import Image
    tree, images = tmp_path / "tree", tmp_path / "images"
    for d in ("mean", "cov", "cov_epistemic", "cat_param"):
        (tree / d).mkdir(parents=True)
    images.mkdir()
    rng = np.random.RandomState(5)
    names, frames, labels = [], [], []
    for i, (h, w) in enumerate([(40, 56), (33, 47), (40, 56)]):
        name = "frame%d" % i
        k = (3, 0, 2)[i]
        v, u = rng.uniform(10, h - 10, k), rng.uniform(10, w - 10, k)        # corners stay inside the frame: HEAT accepts every row
        mean = np.stack([v, u, rng.uniform(6, 16, k), rng.uniform(6, 16, k)], axis=1)
        a = rng.uniform(-1, 1, (k, 4, 4))
        cov = np.matmul(a, a.transpose(0, 2, 1)) + 0.5 * np.eye(4)
        cat = rng.dirichlet(np.ones(8) * 0.3, k).reshape(k, 8)
        np.save(tree / "mean" / (name + ".npy"), mean)
        np.save(tree / "cov" / (name + ".npy"), cov)
        np.save(tree / "cov_epistemic" / (name + ".npy"), 0.3 * cov)
        np.save(tree / "cat_param" / (name + ".npy"), cat)
        f = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        Image.fromarray(f).save(str(images / (name + ".png")))
        names.append(name)
        frames.append(f)
        labels.append({"name": name + ".png", "labels": [{"category": "car", "box2d": {"x1": 4.0, "y1": 5.0, "x2": 30.5, "y2": 28.0}}]})
    (tmp_path / "val.json").write_text(json.dumps(labels))
    return str(tree), str(images), names, frames


def test_show_predictions_writes_what_render_frames_gives(tmp_path, capsys):
    from PIL import Image
    from bayes_od_rc_amd import render, show_predictions
    tree, images, names, frames = _tree(tmp_path)
    out = tmp_path / "out"
    rc = show_predictions.main(["--predictions", tree, "--images", images, "--out", str(out), "--labels", str(tmp_path / "val.json"),
                                "--view", "both", "--min_score", "0.0", "--cov_scale", "4.0", "--line_width", "3", "--gpu-device", "0"])
    assert rc == 0 and "6 files" in capsys.readouterr().out
    assert sorted(os.listdir(out)) == sorted("%s_%s.png" % (n, v) for n in names for v in ("overlay", "heat"))
    dets = [render.detections_from_tree(tree, n, min_score=0.0, cov_scale=4.0, categories=CATEGORIES) for n in names]
    assert [len(d.boxes) for d in dets] == [3, 0, 2]
    gt = [np.array([[4, 5, 30, 28]], np.int32)] * 3
    for view in ("overlay", "heat"):
        want = render.render_frames(frames, dets, view=view, line_width=3, gt_boxes=gt)
        for n, w in zip(names, want):
            got = np.asarray(Image.open(str(out / ("%s_%s.png" % (n, view)))).convert("RGB"))
            assert np.array_equal(got, w), (n, view)
        assert (want[0] != frames[0]).any()
    # one part of a --covariance_parts tree, the first two frames only, in batches of one: different ellipses, same boxes
    part = tmp_path / "part"
    show_predictions.main(["--predictions", tree, "--images", images, "--out", str(part), "--cov_dir", "cov_epistemic", "--frames", "2",
                           "--batch", "1", "--min_score", "0.0", "--cov_scale", "4.0", "--line_width", "3"])
    assert sorted(os.listdir(part)) == ["frame0_overlay.png", "frame1_overlay.png"]
    a = np.asarray(Image.open(str(part / "frame0_overlay.png")))
    b = np.asarray(Image.open(str(out / "frame0_overlay.png")))
    assert a.shape == b.shape and (a != b).any()


def _bdd_dataset(tmp_path):
    from PIL import Image
    root = tmp_path / "bdd100k"
    (root / "images" / "100k" / "val").mkdir(parents=True)
    (root / "labels").mkdir()
    rng = np.random.RandomState(2)
    y, x = np.mgrid[0:128, 0:128]
    names = []
    for i in range(2):
        f = np.clip(np.stack([x + 20 * i, 2 * y, 255 - x], axis=-1) + rng.randint(-30, 31, (128, 128, 3)), 0, 255).astype(np.uint8)
        Image.fromarray(f).save(str(root / "images" / "100k" / "val" / ("f%d.jpg" % i)), format="JPEG", quality=92, subsampling=0)
        names.append("f%d" % i)
    (root / "labels" / "val.json").write_text(json.dumps([]))
    return root, names


def test_run_inference_render(tmp_path, monkeypatch):
    import yaml
    from PIL import Image
    from bayes_od_rc_amd import config_utils, run_inference, synthetic
    from bayes_od_rc_amd.model import RetinaNetModel
    here = os.path.dirname(os.path.abspath(run_inference.__file__))
    weights = str(tmp_path / "weights.npz")
    RetinaNetModel.save_weights_npz(synthetic.make_weights(8, 9, cls_fg_bias=-1.0), weights)
    monkeypatch.setenv("BAYESOD_DATA_DIR", str(tmp_path / "synthetic"))
    out = tmp_path / "drawn"
    tree = run_inference.main(["--gpu_device", "0", "--data_split", "test", "--synthetic", "3", "--image_size", "128", "128", "--batch", "2",
                               "--weights", weights, "--render", str(out), "--render_min_score", "0.0"])
    assert sorted(os.listdir(out)) == ["%06d_overlay.png" % i for i in range(3)]
    drawn = 0
    for i in range(3):
        src = np.random.default_rng(i).integers(0, 256, size=(128, 128, 3), dtype=np.uint8)     # what make_frames normalised
        got = np.asarray(Image.open(str(out / ("%06d_overlay.png" % i))))
        k = np.load(os.path.join(tree, "mean", "%06d.npy" % i)).shape[0]
        assert got.shape == src.shape and ((got != src).any() == (k > 0))
        drawn += k
    assert drawn > 0
    # --dataset, the JPEG files travelling as bytes: both views of both frames
    root, names = _bdd_dataset(tmp_path)
    cfg = config_utils.load_yaml(os.path.join(here, "configs", "retinanet_bdd_covar.yaml"))
    cfg["dataset_config"]["bdd"]["paths_config"]["dataset_dir"] = str(root)
    ypath = tmp_path / "retinanet_bdd_covar.yaml"          # the file name must equal checkpoint_name
    ypath.write_text(yaml.safe_dump(cfg))
    monkeypatch.setenv("BAYESOD_DATA_DIR", str(tmp_path / "dataset"))
    out2 = tmp_path / "drawn2"
    run_inference.main(["--gpu_device", "0", "--yaml_path", str(ypath), "--data_split", "test", "--dataset", "--weights", weights, "--batch", "2",
                        "--device_jpeg", "--render", str(out2), "--render_view", "both", "--render_min_score", "0.9"])
    assert sorted(os.listdir(out2)) == sorted("%s_%s.png" % (n, v) for n in names for v in ("overlay", "heat"))
    for n in names:
        assert np.asarray(Image.open(str(out2 / (n + "_heat.png")))).shape == (128, 128, 3)
