"""GPU: batches of mixed source sizes -- bod_upload_frames_u8_ragged[_async] (every frame resized / padded by its own geometry,
bit-exact against the uniform route and oracle/preprocess.py), every frame's own S = orig / net in the posterior, the pipelined
form, training and validation handles, and --mixed_sizes of run_inference / run_validation on a KITTI tree.

Network input 128x416 (the existing KITTI tests' size).  Source sizes: (94,310) one pad row, up-scaling; (92,306) three pad
rows split 1 / 2; (96,312) no padding; (60,300) 45 pad rows; (200,150) 320 pad columns, down-scaling."""
import os

import numpy as np
import pytest

from conftest import ANCHOR_CFG, BAYES_CFG, NMS_CFG

pytestmark = pytest.mark.gpu

HW = (128, 416)
FIVE = [(94, 310), (92, 306), (96, 312), (60, 300), (200, 150)]
THREE = [(94, 310), (92, 306), (60, 300)]
SEED, FIRST = 4, 20


def _u8(sizes, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, size=hw + (3,), dtype=np.uint8) for hw in sizes]


def _kitti_means():
    from bayes_od_rc_amd import constants
    return constants.MEANS_DICT['Kitti']


def _same_detections(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


def test_ragged_preprocessing_is_bit_exact():
    from bayes_od_rc_amd import datasets
    from bayes_od_rc_amd.engine import Engine, make_config
    from oracle import preprocess as pp
    frames = _u8(FIVE, 1)
    eng = Engine(make_config(HW, batch=5, mc_samples=2))
    eng.upload_frames_u8_ragged(frames, _kitti_means(), aspect_resize=True)
    got = eng.get_images()
    for b, f in enumerate(frames):
        ref = pp.kitti_preprocess(f, HW, _kitti_means())
        assert got[b].shape == ref.shape
        assert np.array_equal(got[b], ref), (b, float(np.abs(got[b] - ref).max()))
    # ... and every frame equals the same slot of a uniform upload of five copies of it
    for b, f in enumerate(frames):
        eng.upload_frames_u8(np.stack([f] * 5), _kitti_means(), aspect_resize=True)
        assert np.array_equal(eng.get_images()[b], got[b]), b
    assert np.array_equal(datasets.normalized_on_device(eng, frames, 'Kitti', aspect_resize=True), got)      # a list goes up ragged
    # no resize: frames at the network size, the BDD handler's normalisation
    flat = _u8([HW] * 5, 2)
    eng.upload_frames_u8_ragged(flat, aspect_resize=False)
    got = eng.get_images()
    for b, f in enumerate(flat):
        assert np.array_equal(got[b], pp.bdd_preprocess(f)), b
    # refusals name the frame, and leave the handle and its frames as they were
    with pytest.raises(ValueError, match="frame 3"):
        eng.upload_frames_u8_ragged(flat[:3] + [flat[3][:100]] + flat[4:], aspect_resize=False)
    with pytest.raises(ValueError, match="frame 1.*degenerate"):
        eng.upload_frames_u8_ragged([flat[0], np.zeros((1, 2000, 3), np.uint8)] + flat[2:], aspect_resize=True)
    with pytest.raises(ValueError, match="expected 5 frames"):
        eng.upload_frames_u8_ragged(flat[:4])
    with pytest.raises(ValueError, match="buffer must be 0 or 1"):
        eng.upload_frames_u8_ragged_async(flat, 2)
    assert np.array_equal(eng.get_images(), got)
    eng.upload_frames_u8_ragged(frames, _kitti_means(), aspect_resize=True)
    assert np.array_equal(eng.get_images()[4], pp.kitti_preprocess(frames[4], HW, _kitti_means()))
    eng.close()


class _Ctx(object):
    pass


@pytest.fixture(scope="module")
def kitti3():
    """A KITTI pipeline of batch 3 (N = 4) and, computed ONCE on the handle while it is fresh, the uniform route's detections
    of every frame: all three slots hold frame b, the pipeline is bound to frame b's size."""
    from bayes_od_rc_amd.anchor_generator import FpnAnchorGenerator
    from bayes_od_rc_amd.inference_utils import BayesOdPipeline
    from test_gpu_pipeline import _model
    c = _Ctx()
    c.frames = _u8(THREE, 3)
    anchors = FpnAnchorGenerator(ANCHOR_CFG).generate_all((HW[0], HW[1], 3))
    c.pipe = BayesOdPipeline(_model(4), HW, 3, BAYES_CFG, NMS_CFG, dataset_name="kitti", orig_size=THREE[0], anchors=anchors)
    c.uniform = [_uniform(c, b) for b in range(3)]
    return c


def _uniform(c, b):
    c.pipe.bind(orig_size=THREE[b])
    c.pipe.engine.upload_frames_u8(np.stack([c.frames[b]] * 3), _kitti_means(), aspect_resize=True)
    return [tuple(x.copy() for x in d) for d in c.pipe(None, seed=SEED, first_image_id=FIRST)]


def test_every_frame_is_rescaled_by_its_own_size(kitti3):
    """Slot b of the ragged batch == slot b of the uniform batch of three copies of frame b bound to orig_size = size_b
    (same seed, same first_image_id, so slot b draws the same Philox streams): array_equal."""
    c = kitti3
    c.pipe.bind(orig_size=(370, 1224))                       # whatever the handle's own pair says: the frames' factors apply
    c.pipe.upload_mixed(c.frames, _kitti_means())
    got = c.pipe(None, seed=SEED, first_image_id=FIRST)
    for b in range(3):
        print("frame", b, THREE[b], "detections", len(got[b][1]), "uniform", len(c.uniform[b][b][1]))
        assert len(c.uniform[b][b][1]) >= 1
        assert _same_detections(got[b], c.uniform[b][b]), b


def test_no_stale_factors_after_a_ragged_batch(kitti3):
    c = kitti3
    c.pipe.upload_mixed(c.frames, _kitti_means())
    c.pipe(None, seed=SEED, first_image_id=FIRST)
    again = _uniform(c, 0)                                   # c.uniform[0] ran on the handle before any ragged upload
    for b in range(3):
        assert _same_detections(again[b], c.uniform[0][b]), b
    # host float frames clear them as well
    from oracle import preprocess as pp
    c.pipe.upload_mixed(c.frames, _kitti_means())
    c.pipe.bind(orig_size=THREE[0])
    floats = np.stack([pp.kitti_preprocess(c.frames[0], HW, _kitti_means())] * 3)
    host = c.pipe(floats, seed=SEED, first_image_id=FIRST)
    for b in range(3):
        assert _same_detections(host[b], c.uniform[0][b]), b


def test_pipelined_ragged_upload_equals_the_synchronous_one():
    """Three clips of mixed sizes through image buffers 0 / 1 / 0 with infer_async, the upload of clip i+1 enqueued under clip
    i: clip by clip the detections of the synchronous ragged route.  Neighbouring clips differ in their sizes slot by slot, so
    factors read from the upload's table after the next upload rewrote it would show."""
    from bayes_od_rc_amd import synthetic
    from bayes_od_rc_amd.anchor_generator import FpnAnchorGenerator
    from bayes_od_rc_amd.engine import Engine, make_config
    batch, n = 2, 3
    eng = Engine(make_config(HW, batch=batch, mc_samples=n, bayes_od_config=BAYES_CFG, nms_config=NMS_CFG, use_full_covar=True,
                             dataset_name="kitti", orig_size=HW))
    eng.load_weights(synthetic.make_weights(cls_fg_bias=-1.0))
    eng.set_anchors(FpnAnchorGenerator(ANCHOR_CFG).generate_all((HW[0], HW[1], 3)))
    sizes = [[(94, 310), (92, 306)], [(60, 300), (96, 312)], [(92, 306), (200, 150)]]
    clips = [_u8(s, 10 + i) for i, s in enumerate(sizes)]
    sync = []
    for i, c in enumerate(clips):
        eng.upload_frames_u8_ragged(c, _kitti_means())
        eng.infer(None, seed=2, first_image_id=batch * i)
        sync.append({k: v.copy() for k, v in eng.get_detections_batch().items()})
    got, pending = [], []
    eng.upload_frames_u8_ragged_async(clips[0], 0, _kitti_means())
    for i in range(len(clips)):
        pending.append(eng.infer_async(None, seed=2, first_image_id=batch * i, image_buffer=i & 1))
        if i + 1 < len(clips):
            eng.upload_frames_u8_ragged_async(clips[i + 1], (i + 1) & 1, _kitti_means())
        if len(pending) > 1:
            got.append({k: v.copy() for k, v in eng.collect(pending.pop(0)).items()})
    got.append({k: v.copy() for k, v in eng.collect(pending.pop(0)).items()})
    assert len(got) == len(sync)
    for a, b in zip(sync, got):
        print("detections per frame", a["num"].tolist(), b["num"].tolist())
        assert np.array_equal(a["num"], b["num"]) and a["num"].min() > 0
        for img in range(batch):
            k = a["num"][img]
            for key in ("scores", "means", "covs", "counts"):
                assert np.array_equal(a[key][img, :k], b[key][img, :k])
    eng.close()


def _gt():
    """One KITTI-shaped ground-truth row per frame: a car, in network pixels (y1, x1, y2, x2)."""
    boxes = [np.asarray([[30.0, 120.0, 94.0, 248.0]], np.float32), np.asarray([[40.0, 200.0, 100.0, 300.0]], np.float32)]
    classes = [np.eye(8, dtype=np.float32)[:1], np.eye(8, dtype=np.float32)[:1]]
    return boxes, classes


def test_validation_handle_takes_a_ragged_upload():
    from bayes_od_rc_amd import synthetic
    from bayes_od_rc_amd.anchor_generator import FpnAnchorGenerator
    from bayes_od_rc_amd.engine import Engine, make_config
    from oracle import preprocess as pp
    frames = _u8([(94, 310), (60, 300)], 6)
    floats = np.stack([pp.kitti_preprocess(f, HW, _kitti_means()) for f in frames])
    boxes, classes = _gt()
    eng = Engine(make_config(HW, batch=2, mc_samples=1, nms_config=NMS_CFG))
    eng.load_weights(synthetic.make_weights(cls_fg_bias=-1.0))
    eng.set_anchors(FpnAnchorGenerator(ANCHOR_CFG).generate_all((HW[0], HW[1], 3)))
    ref_sums, ref_dets = eng.validate_boxes(floats, boxes, classes, 0.5, 0.4)
    eng.upload_frames_u8_ragged(frames, _kitti_means())
    sums, dets = eng.validate_boxes(None, boxes, classes, 0.5, 0.4)
    print("sums", sums.tolist(), "detections", [len(d[1]) for d in dets])
    assert np.isfinite(sums).all() and (sums[:, 3] >= 1).all()
    assert sums.tobytes() == ref_sums.tobytes()
    assert max(len(d[1]) for d in dets) >= 1
    for (c0, b0), (c1, b1) in zip(dets, ref_dets):
        assert np.array_equal(c0, c1) and np.array_equal(b0, b1)
    eng.close()


def test_training_handle_takes_a_ragged_upload():
    """The three losses that depend on the frames -- classification, regression, covariance -- are bitwise those of the step on
    the oracle-preprocessed float frames.  The regularisation term does not read the frames at all, and the step adds it up with
    float atomics in the order the workgroups happen to finish (fold_pack's l2_loss), so two runs of ANY route differ in its
    last bits (measured here: 2 ulp of 0.0052); it is held to 1e-5, the bound tests/test_gpu_validation_boxes.py holds the
    same quantity to, and the total to the sum of its parts."""
    from bayes_od_rc_amd import synthetic
    from bayes_od_rc_amd.anchor_generator import FpnAnchorGenerator
    from bayes_od_rc_amd.engine import Engine, make_config
    from oracle import preprocess as pp
    frames = _u8([(94, 310), (60, 300)], 6)
    floats = np.stack([pp.kitti_preprocess(f, HW, _kitti_means()) for f in frames])
    boxes, classes = _gt()
    eng = Engine(make_config(HW, batch=2, mc_samples=1, training=True))
    eng.load_weights(synthetic.make_weights(cls_fg_bias=-2.0))
    eng.set_anchors(FpnAnchorGenerator(ANCHOR_CFG).generate_all((HW[0], HW[1], 3)))
    ref = eng.train_step_boxes(floats, boxes, classes, 0.5, 0.4, seed=3, first_image_id=8, apply_update=False)
    eng.upload_frames_u8_ragged(frames, _kitti_means())
    got = eng.train_step_boxes(None, boxes, classes, 0.5, 0.4, seed=3, first_image_id=8, apply_update=False)
    print("losses", got)
    assert np.isfinite(got["total_loss"]) and got["reg_loss"] > 0
    for key in ("cls_loss", "reg_loss", "covariance_loss"):
        assert got[key] == ref[key], (key, got[key], ref[key])
    assert abs(got["regularization_loss"] - ref["regularization_loss"]) <= 1e-5 * ref["regularization_loss"]
    for out in (got, ref):
        assert out["total_loss"] == out["cls_loss"] + 1.0 * (out["reg_loss"] + out["covariance_loss"]) + out["regularization_loss"]
    eng.close()


def _kitti_tree(tmp_path, split):
    """Five frames with sizes A, B, A, B, A and one label row each (the tree of test_run_inference_on_a_kitti_tree)."""
    from PIL import Image
    root = tmp_path / "object"
    (root / "training" / "image_2").mkdir(parents=True)
    (root / "training" / "label_2").mkdir()
    ids = ["%06d" % i for i in range(5)]
    (root / (split + ".txt")).write_text("\n".join(ids) + "\n")
    rng = np.random.default_rng(5)
    for i, sid in enumerate(ids):
        hw = (94, 310) if i % 2 == 0 else (92, 306)
        Image.fromarray(rng.integers(0, 256, size=hw + (3,), dtype=np.uint8)).save(str(root / "training" / "image_2" / (sid + ".png")))
        (root / "training" / "label_2" / (sid + ".txt")).write_text(
            "Car 0.00 0 -1.57 100.00 20.00 200.00 80.00 1.5 1.6 3.9 1.0 1.5 10.0 -1.5\n")
    return root, ids


def _yaml(tmp_path, root, edit):
    import yaml
    from bayes_od_rc_amd import config_utils, run_inference
    here = os.path.dirname(os.path.abspath(run_inference.__file__))
    cfg = config_utils.load_yaml(os.path.join(here, "configs", "retinanet_bdd_covar.yaml"))
    cfg["dataset_config"]["kitti"]["paths_config"]["dataset_dir"] = str(root)
    cfg["dataset_config"]["kitti"]["resize_shape"] = [128, 416]
    edit(cfg)
    ypath = tmp_path / "retinanet_bdd_covar.yaml"          # the file name must equal checkpoint_name
    ypath.write_text(yaml.safe_dump(cfg))
    return str(ypath)


def test_run_inference_mixed_sizes_equals_the_default_route(tmp_path, monkeypatch):
    from bayes_od_rc_amd import run_inference, synthetic
    from bayes_od_rc_amd.model import RetinaNetModel
    root, ids = _kitti_tree(tmp_path, "test")
    weights = str(tmp_path / "weights.npz")                  # (the default synthetic class bias, -4.6, detects nothing on these frames)
    RetinaNetModel.save_weights_npz(synthetic.make_weights(8, 9, cls_fg_bias=-1.0), weights)

    def edit(cfg):
        cfg["testing_config"]["test_dataset"] = "kitti"
    ypath = _yaml(tmp_path, root, edit)
    args = ["--gpu_device", "0", "--yaml_path", ypath, "--data_split", "test", "--dataset", "--batch", "4",
            "--weights", weights]
    monkeypatch.setenv("BAYESOD_DATA_DIR", str(tmp_path / "default"))
    ref = run_inference.main(args)
    monkeypatch.setenv("BAYESOD_DATA_DIR", str(tmp_path / "mixed"))
    out = run_inference.main(args + ["--mixed_sizes"])
    assert ref != out and os.path.join("predictions", "testing", "kitti") in out
    total = 0
    for sid in ids:
        for kind in ("mean", "cov", "cat_param", "cat_count"):
            a, b = np.load(os.path.join(ref, kind, sid + ".npy")), np.load(os.path.join(out, kind, sid + ".npy"))
            assert a.shape == b.shape and np.array_equal(a, b), (sid, kind)
        total += np.load(os.path.join(out, "mean", sid + ".npy")).shape[0]
        with open(os.path.join(ref, "data", sid + ".txt")) as fa, open(os.path.join(out, "data", sid + ".txt")) as fb:
            assert fa.read() == fb.read(), sid
    print("detections over the five frames:", total)
    assert total >= 5


def test_run_validation_mixed_sizes_equals_the_bucketed_route(tmp_path, monkeypatch):
    from bayes_od_rc_amd import run_validation
    from test_gpu_validation_boxes import _checkpoint
    root, ids = _kitti_tree(tmp_path, "val")

    def edit(cfg):
        cfg["dataset_config"]["dataset"] = "kitti"
    ypath = _yaml(tmp_path, root, edit)
    real_batch = run_validation.validate_batch
    results = {}
    for route, flag in (("bucketed", []), ("mixed", ["--mixed_sizes"])):
        (tmp_path / route).mkdir()
        monkeypatch.setenv("BAYESOD_DATA_DIR", str(tmp_path / route / "data"))
        _checkpoint(tmp_path / route, 4)
        seen, frames = [], {}

        def watched_batch(model, config, batch, **kw):
            out = real_batch(model, config, batch, **kw)
            seen.append(tuple(tuple(int(v) for v in s["im_size"][:2]) for s in batch))
            for s, (total, loss_dict, classes, corners) in zip(batch, out):
                frames[s["image_uint8"].tobytes()] = (float(total), dict(loss_dict), classes.copy(), corners.copy())
            return out
        monkeypatch.setattr(run_validation, "validate_batch", watched_batch)
        res = run_validation.main(["--gpu_device", "0", "--yaml_path", ypath, "--data_split", "val", "--dataset", "--batch", "4"] + flag)
        monkeypatch.setattr(run_validation, "validate_batch", real_batch)
        assert len(res) == 1 and res[0]["num_frames"] == 5
        out_dir = os.path.join(str(tmp_path / route / "data"), "outputs", "retinanet_bdd_covar", "predictions", "validation", "1", "data")
        texts = {sid: open(os.path.join(out_dir, sid + ".txt")).read() for sid in ids}
        results[route] = (res[0], seen, frames, texts)
    a, b = (94, 310), (92, 306)
    assert results["bucketed"][1] == [(b, b), (a, a, a)]                   # the partial buckets, flushed by size
    assert results["mixed"][1] == [(a, b, a, b), (a,)]                     # one pass in dataset order, one tail batch
    fa, fb = results["bucketed"][2], results["mixed"][2]
    assert set(fa) == set(fb) and len(fa) == 5
    for key in fa:
        assert fa[key][0] == fb[key][0] and fa[key][1] == fb[key][1]
        assert np.array_equal(fa[key][2], fb[key][2]) and np.array_equal(fa[key][3], fb[key][3])
    assert results["bucketed"][3] == results["mixed"][3]
    ra, rb = results["bucketed"][0], results["mixed"][0]
    print("validation", ra["mean_total_loss"], rb["mean_total_loss"], ra["num_detections"], rb["num_detections"])
    assert ra["num_detections"] == rb["num_detections"] >= 1
    assert ra["mean_total_loss"] == rb["mean_total_loss"]
