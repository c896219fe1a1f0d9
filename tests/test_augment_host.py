"""CPU: the host side of training-time augmentation -- bod_augment_boxes (pure host code: called through the shared library, which
loads without a device) against the float32 restatement of tests/augment_reference.py, the host geometry at off = 0.5 against
the centred offsets of oracle/preprocess.py, draw_augmentation's streams, run_training --augment with a stub engine, and the
declarations of the three entry points."""
import os
import re

import numpy as np
import pytest

from augment_reference import augmented_boxes, geometry, record
from conftest import ROOT

NAMES = ("bod_upload_frames_u8_augmented", "bod_upload_frames_u8_augmented_async", "bod_augment_boxes")
NET = (128, 416)


def _classes(n, width=4, seed=0):
    return np.eye(width, dtype=np.float32)[np.random.default_rng(seed).integers(0, width - 1, n)]


def _check(sizes, net, aspect, recs, boxes, classes, min_visible):
    from bayes_od_rc_amd.engine import augment_boxes
    got_b, got_c = augment_boxes(sizes, net, recs, boxes, classes, aspect_resize=aspect, min_visible=min_visible)
    assert len(got_b) == len(got_c) == len(sizes)
    for i in range(len(sizes)):
        want_b, want_c = augmented_boxes(sizes[i], net, aspect, recs[i], boxes[i], classes[i], min_visible)
        assert got_b[i].dtype == np.float32 and got_b[i].shape == want_b.shape, (i, got_b[i], want_b)
        assert got_b[i].tobytes() == want_b.tobytes(), (i, got_b[i], want_b)
        assert np.array_equal(got_c[i], want_c), i
        assert got_b[i].shape[0] >= 1
    return got_b, got_c


def test_identity_flip_and_mixed_sizes_against_the_restatement():
    sizes = [(94, 311), (92, 306), (200, 150), (100, 500)]                     # odd / even width, narrower / wider than the network
    rng = np.random.default_rng(1)
    boxes, classes = [], []
    for i, (h, w) in enumerate(sizes):
        y1, x1 = rng.uniform(0, h * 0.5, 3), rng.uniform(0, w * 0.5, 3)
        boxes.append(np.stack([y1, x1, y1 + rng.uniform(8, h * 0.45, 3), x1 + rng.uniform(8, w * 0.45, 3)], 1).astype(np.float32))
        classes.append(_classes(3, seed=i))
    ident = [record() for _ in sizes]
    got, _ = _check(sizes, NET, True, ident, boxes, classes, 0.25)
    assert all(g.shape == (3, 4) for g in got)                                   # nothing leaves a centred, unscaled frame
    flipped = [record(flip=1) for _ in sizes]
    _check(sizes, NET, True, flipped, boxes, classes, 0.25)
    _check(sizes, NET, True, [record(flip=i & 1, scale=s, off_y=0.37, off_x=1.0, gain=1.3, bias=-7.0)
                              for i, s in enumerate((0.7, 1.4, 1.4, 0.5))], boxes, classes, 0.25)
    # no resize: frames at the network size (the BDD route), scaled about themselves
    flat = [NET] * 2
    fb = [np.asarray([[10, 20, 100, 300], [5, 5, 60, 80]], np.float32)] * 2
    _check(flat, NET, False, [record(scale=0.75, off_y=0.0, off_x=1.0), record(flip=1, scale=1.3)], fb, [_classes(2)] * 2, 0.25)


def test_flip_twice_returns_the_input_exactly():
    """Boxes with integer corners in the SOURCE frame: (w-1) - x is exact, so two flips of the source give the input bit for bit.
    The frame is at the network size and unscaled, so the rest of the map is x * 1 + 0."""
    from bayes_od_rc_amd.engine import augment_boxes
    boxes = [np.asarray([[3, 7, 90, 200], [0, 0, 127, 415], [50, 400, 70, 415]], np.float32)]
    classes = [_classes(3)]
    once, c1 = augment_boxes([NET], NET, [record(flip=1)], boxes, classes, aspect_resize=False, min_visible=0.0)
    assert np.array_equal(once[0][:, 1], 415 - boxes[0][:, 3]) and np.array_equal(once[0][:, 3], 415 - boxes[0][:, 1])
    assert np.array_equal(once[0][:, [0, 2]], boxes[0][:, [0, 2]])
    twice, c2 = augment_boxes([NET], NET, [record(flip=1)], once, c1, aspect_resize=False, min_visible=0.0)
    assert twice[0].tobytes() == boxes[0].tobytes() and np.array_equal(c2[0], classes[0])


def test_scale_and_crop_drop_by_min_visible_and_keep_at_the_boundary():
    """Network 129x129, a 129x129 frame scaled by 2 (no aspect resize: 258x258) and cropped at offset 0, so the clip limit is
    128.  The box from 32 to 96 maps to 64..192 and keeps 64..128 of it: 64 * 64 of 128 * 128, exactly 0.25.  With min_visible
    = 0.25 it is KEPT (not below the bound); one float32 step above, it is dropped.  The box from 100 to 120 lies outside the
    crop altogether (clipped height 0), the third one inside it."""
    net = (129, 129)
    boxes = [np.asarray([[32, 32, 96, 96], [100, 100, 120, 120], [5, 5, 25, 45]], np.float32)]
    classes = [np.eye(4, dtype=np.float32)[[0, 1, 2]]]
    rec = [record(scale=2.0, off_y=0.0, off_x=0.0)]
    assert geometry(net, net, False, 2.0, 0.0, 0.0) == (258, 258, 0, 0, 0, 0)
    got_b, got_c = _check([net], net, False, rec, boxes, classes, 0.25)
    assert np.array_equal(got_b[0], np.asarray([[64, 64, 128, 128], [10, 10, 50, 90]], np.float32))
    assert np.array_equal(got_c[0], classes[0][[0, 2]])
    above = float(np.nextafter(np.float32(0.25), np.float32(1)))
    got_b, got_c = _check([net], net, False, rec, boxes, classes, above)
    assert np.array_equal(got_b[0], np.asarray([[10, 10, 50, 90]], np.float32)) and np.array_equal(got_c[0], classes[0][[2]])
    # the same frame cropped at offset 1 (crop 129): only the box that was outside stays
    assert geometry(net, net, False, 2.0, 1.0, 1.0) == (258, 258, 129, 129, 0, 0)
    got_b, got_c = _check([net], net, False, [record(scale=2.0, off_y=1.0, off_x=1.0)], boxes, classes, 0.5)
    assert np.array_equal(got_b[0], np.asarray([[71, 71, 111, 111]], np.float32)) and np.array_equal(got_c[0], classes[0][[1]])


def test_a_frame_that_loses_every_box_gets_the_placeholder_row():
    from bayes_od_rc_amd.engine import augment_boxes
    net = (100, 100)
    boxes = [np.asarray([[60, 60, 90, 90]], np.float32), np.asarray([[10, 10, 40, 40]], np.float32), np.zeros((0, 4), np.float32)]
    classes = [np.eye(4, dtype=np.float32)[[1]], np.eye(4, dtype=np.float32)[[0]], np.zeros((0, 4), np.float32)]
    recs = [record(scale=2.0, off_y=0.0, off_x=0.0), record(), record()]
    got_b, got_c = augment_boxes([net] * 3, net, recs, boxes, classes, aspect_resize=False, min_visible=0.25)
    for i in (0, 2):                                                            # cropped away / no ground truth to begin with
        assert np.array_equal(got_b[i], np.asarray([[0, 0, 1, 1]], np.float32))
        assert np.array_equal(got_c[i], np.asarray([[0, 0, 0, 1]], np.float32))
    assert np.array_equal(got_b[1], boxes[1]) and np.array_equal(got_c[1], classes[1])
    _check([net] * 2, net, False, recs[:2], boxes[:2], classes[:2], 0.25)


def test_refusals_name_the_frame():
    from bayes_od_rc_amd.engine import augment_boxes
    b, c = [np.asarray([[1, 1, 20, 20]], np.float32)] * 2, [_classes(1)] * 2
    for bad in (dict(flip=2), dict(scale=0.0), dict(scale=-1.0), dict(scale=float("nan")), dict(scale=float("inf")),
                dict(off_y=-0.01), dict(off_x=1.5), dict(off_y=float("nan")), dict(gain=float("inf")), dict(bias=float("nan")),
                dict(scale=1e9)):
        with pytest.raises(ValueError, match="bod_augment_boxes: frame 1"):
            augment_boxes([(94, 310)] * 2, NET, [record(), record(**bad)], b, c)
    with pytest.raises(ValueError, match="frame 0 is 94x310"):
        augment_boxes([(94, 310)] * 2, NET, [record()] * 2, b, c, aspect_resize=False)
    with pytest.raises(ValueError, match="frame 1.*degenerate"):
        augment_boxes([(94, 310), (1, 2000)], NET, [record()] * 2, b, c)


def test_centred_offsets_are_the_existing_ones():
    """off = 0.5: floor(0.5 d) is the d // 2 of tf.image.resize_with_crop_or_pad for every size difference d, pad or crop.  The
    host geometry is seen through the map of one box, the middle third of the source frame: box * ratio + pad - crop, clipped,
    with the size of oracle/preprocess.py's preserve_aspect_size and the offsets of its crop_or_pad_offsets.  Scale 1 is the
    geometry of every other upload; the other two scales bring crops in."""
    import math
    from bayes_od_rc_amd.engine import augment_boxes
    from oracle import preprocess as pp
    f = np.float32
    nets = [(128, 416), (64, 64), (65, 97), (33, 70), (300, 40)]
    sources = [(94, 310), (92, 306), (93, 307), (60, 300), (200, 150), (375, 1242), (370, 1224), (31, 33), (70, 1000), (500, 90)]
    n, seen = 0, set()
    for net in nets:
        for src in sources + [net]:
            for aspect in (True, False):
                if not aspect and src != net:
                    continue
                for scale in (1.0, 1.37, 0.61):
                    s = float(f(scale))
                    if aspect:
                        rh, rw = pp.preserve_aspect_size(src, tuple(max(1, int(math.floor(s * v + 0.5))) for v in net))
                    else:
                        rh, rw = (max(1, int(math.floor(s * v + 0.5))) for v in src)
                    cy, cx, py, px = pp.crop_or_pad_offsets((rh, rw), net)
                    assert geometry(src, net, aspect, scale) == (rh, rw, cy, cx, py, px)     # the restatement agrees with the oracle
                    box = np.asarray([[src[0] / 3.0, src[1] / 3.0, 2.0 * src[0] / 3.0, 2.0 * src[1] / 3.0]], f)
                    want = box * np.asarray([f(rh / src[0]), f(rw / src[1])] * 2, f) + np.asarray([py - cy, px - cx] * 2, f)
                    want = np.minimum(np.maximum(want, f(0)), np.asarray([net[0] - 1, net[1] - 1] * 2, f))
                    if want[0, 2] - want[0, 0] < 1 or want[0, 3] - want[0, 1] < 1:
                        continue                                                # (a resized frame of a few pixels: the box would be dropped)
                    got, _ = augment_boxes([src], net, [record(scale=scale)], [box], [np.asarray([[1, 0]], f)], aspect_resize=aspect,
                                           min_visible=0.0)
                    assert got[0].tobytes() == want.tobytes(), (src, net, aspect, scale, got[0], want)
                    n += 1
                    seen.add((int(np.sign(rh - net[0])), (rh - net[0]) % 2))
                    seen.add((int(np.sign(rw - net[1])), (rw - net[1]) % 2))
    assert n >= 150
    assert seen >= {(-1, 0), (-1, 1), (1, 0), (1, 1), (0, 0)}                  # odd and even differences, padded and cropped


def test_draws_depend_on_seed_and_image_id_alone():
    from bayes_od_rc_amd.engine import AUGMENT_DEFAULTS, AUGMENT_DTYPE, draw_augmentation
    a = draw_augmentation(None, 7, range(12))
    assert a.dtype == AUGMENT_DTYPE and a.shape == (12,) and AUGMENT_DTYPE.itemsize == 24
    # whatever the batch it sits in: batches of 4 (a resumed run starts at any of them), a rank's strided share, one by one
    for lo in (0, 4, 8):
        assert draw_augmentation(None, 7, range(lo, lo + 4)).tobytes() == a[lo:lo + 4].tobytes()
    assert draw_augmentation(None, 7, [9, 2, 5]).tobytes() == a[[9, 2, 5]].tobytes()
    assert draw_augmentation(dict(AUGMENT_DEFAULTS), 7, [3]).tobytes() == a[3:4].tobytes()
    # different ids, and different seeds, differ
    assert len(set(r.tobytes() for r in a)) == 12
    assert draw_augmentation(None, 8, range(12)).tobytes() != a.tobytes()
    # the documented order of the six draws
    u = np.random.Generator(np.random.Philox(key=[7, 5])).random(6)
    r = a[5]
    assert r["flip"] == int(u[0] < 0.5) and r["off_y"] == np.float32(u[2]) and r["off_x"] == np.float32(u[3])
    assert abs(float(r["scale"]) - np.exp(np.log(0.8) + u[1] * (np.log(1.25) - np.log(0.8)))) < 1e-6
    assert abs(float(r["gain"]) - (0.8 + u[4] * 0.4)) < 1e-6 and abs(float(r["bias"]) - (-20 + u[5] * 40)) < 1e-5
    # a switch that is off does not shift the other draws
    calm = draw_augmentation({"flip_probability": 0.0, "random_placement": False, "scale_range": [1.0, 1.0]}, 7, range(12))
    assert not calm["flip"].any() and (calm["off_y"] == 0.5).all() and (calm["off_x"] == 0.5).all() and (calm["scale"] == 1).all()
    assert np.array_equal(calm["gain"], a["gain"]) and np.array_equal(calm["bias"], a["bias"])
    with pytest.raises(ValueError, match="unknown augmentation setting"):
        draw_augmentation({"rotate": 3}, 0, [0])


def test_draws_respect_their_ranges():
    from bayes_od_rc_amd.engine import AUGMENT_DEFAULTS, draw_augmentation
    a = draw_augmentation(None, 3, range(1000))
    d = AUGMENT_DEFAULTS
    for key, rng in (("scale", d["scale_range"]), ("gain", d["gain_range"]), ("bias", d["bias_range"]), ("off_y", (0, 1)), ("off_x", (0, 1))):
        v = a[key].astype(np.float64)
        assert v.min() >= rng[0] and v.max() <= rng[1], (key, v.min(), v.max())
        assert v.max() - v.min() > 0.9 * (rng[1] - rng[0]), key                # ... and fill them
    assert set(a["flip"].tolist()) == {0, 1} and 400 < a["flip"].sum() < 600
    assert abs(np.log(a["scale"].astype(np.float64)).mean() - 0.5 * (np.log(0.8) + np.log(1.25))) < 0.02       # log-uniform
    # bounds that are no float32 (1.2 rounds up, 0.1 rounds up): rounding a draw to float32 must not step over them
    tight = draw_augmentation({"scale_range": [1.1999999, 1.2], "gain_range": [1.1999999, 1.2], "bias_range": [0.0999999, 0.1],
                               "flip_probability": 1.0}, 3, range(50))
    for key, lo, hi in (("scale", 1.1999999, 1.2), ("gain", 1.1999999, 1.2), ("bias", 0.0999999, 0.1)):
        v = tight[key].astype(np.float64)
        assert (v >= lo).all() and (v <= hi).all(), (key, v.min(), v.max())
    assert tight["flip"].all()


def test_records_from_dicts():
    from bayes_od_rc_amd.engine import AUGMENT_DTYPE, augment_records
    r = augment_records([{}, {"flip": 1, "bias": -3.5}], 2)
    assert r.dtype == AUGMENT_DTYPE and r.flags["C_CONTIGUOUS"]
    assert r[0].tolist() == (0, 1.0, 0.5, 0.5, 1.0, 0.0) and r[1].tolist() == (1, 1.0, 0.5, 0.5, 1.0, -3.5)
    assert augment_records(r, 2) is r or augment_records(r, 2).tobytes() == r.tobytes()
    with pytest.raises(ValueError, match="expected 3 augmentation records, got 2"):
        augment_records(r, 3)
    with pytest.raises(ValueError, match="frame 1: unknown"):
        augment_records([{}, {"rotate": 1}])


# ------------------------------------------------------------------------------------------------ run_training with a stub engine
class _StubEngine(object):
    log = []

    def __init__(self, cfg):
        self.cfg, self.B, self._anchors_set = cfg, cfg.batch, False

    def load_weights(self, weights):
        pass

    def set_anchors(self, anchors):
        self._anchors_set = True

    def upload_frames_u8(self, frames, means=None, aspect_resize=False):
        self.log.append(("uniform",))

    def upload_frames_u8_ragged(self, frames, means=None, aspect_resize=True):
        self.log.append(("ragged",))

    def upload_frames_u8_augmented(self, frames, aug, means=None, aspect_resize=True):
        assert len(frames) == self.B and len(aug) == self.B
        self.log.append(("augmented", aug.copy(), [f.shape[:2] for f in frames], bool(aspect_resize)))

    def upload_frames_u8_augmented_async(self, *a, **k):
        self.log.append(("augmented_async",))

    def train_step_boxes(self, images, boxes, classes, *a, **kw):
        self.log.append(("step", images is None, kw["first_image_id"], [np.asarray(b).copy() for b in boxes]))
        return {"total_loss": 1.0, "cls_loss": 0.5, "reg_loss": 0.25, "covariance_loss": 0.125, "regularization_loss": 0.125}


class _StubHandler(object):
    """KITTI-shaped ground-truth-only samples of two sizes, one box each in source pixels."""
    resize_shape = [128, 416]
    epoch_size = 6
    dense_targets = True

    def create_dataset(self):
        from bayes_od_rc_amd import constants
        for i in range(self.epoch_size):
            h, w = ((94, 310), (92, 306))[i & 1]
            src = np.asarray([[10.0, 20.0 + i, 70.0, 200.0]], np.float32)
            yield {constants.IMAGE_NORMALIZED_KEY: None, "image_uint8": np.full((h, w, 3), i, np.uint8),
                   constants.ORIGINAL_IM_SIZE_KEY: np.asarray([h, w, 3], np.int32), constants.ANCHORS_KEY: np.zeros((4, 4), np.float32),
                   constants.BOXES_2D_GT_KEY: src / np.asarray([h, w, h, w], np.float32) * np.asarray([128, 416, 128, 416], np.float32),
                   "boxes_2d_gt_source": src, constants.BOXES_CLASS_GT_KEY: np.asarray([[1, 0, 0, 0]], np.float32)}


@pytest.fixture
def stub_run(monkeypatch, tmp_path):
    from bayes_od_rc_amd import datasets, run_training
    monkeypatch.setenv("BAYESOD_DATA_DIR", str(tmp_path))
    monkeypatch.setattr(run_training, "Engine", _StubEngine)
    monkeypatch.setattr(run_training.synthetic, "make_weights", lambda *a, **k: {})
    monkeypatch.setattr(run_training, "save_checkpoint", lambda trainer, path: None)
    monkeypatch.setattr(datasets, "build_dataset", lambda cfg, split: _StubHandler())
    drawn = []
    real = run_training.draw_augmentation

    def watched(cfg, seed, image_ids):
        drawn.append((dict(cfg), seed, [int(i) for i in image_ids]))
        return real(cfg, seed, image_ids)
    monkeypatch.setattr(run_training, "draw_augmentation", watched)
    _StubEngine.log = []
    return run_training, drawn


def test_run_training_without_the_flag_runs_no_new_code(stub_run):
    run_training, drawn = stub_run
    history, _ = run_training.main(["--dataset", "--steps", "2", "--seed", "5", "--no_resume"])
    assert len(history) == 2 and drawn == []
    kinds = [e[0] for e in _StubEngine.log]
    assert kinds == ["uniform", "step", "uniform", "step"]                      # bucketed by size, as ever
    assert not any(k.startswith("augmented") for k in kinds)


def test_run_training_augment_draws_one_record_per_image_id(stub_run):
    from augment_reference import augmented_boxes as ref_boxes
    from bayes_od_rc_amd.engine import AUGMENT_DEFAULTS, draw_augmentation
    run_training, drawn = stub_run
    history, _ = run_training.main(["--dataset", "--augment", "--steps", "3", "--seed", "5", "--no_resume"])
    assert len(history) == 3
    assert [d[2] for d in drawn] == [[0, 1, 2], [3, 4, 5], [6, 7, 8]]           # step * batch + i (minibatch_size 3)
    assert all(d[0] == AUGMENT_DEFAULTS and d[1] == 5 for d in drawn)
    log = _StubEngine.log
    assert [e[0] for e in log] == ["augmented", "step"] * 3                     # once per step, nothing else goes up
    sizes = [(94, 310), (92, 306)]
    for step in range(3):
        up, st = log[2 * step], log[2 * step + 1]
        want = draw_augmentation(None, 5, range(3 * step, 3 * step + 3))
        assert up[1].tobytes() == want.tobytes() and up[3] is True
        assert up[2] == [sizes[(3 * step + i) & 1] for i in range(3)]           # the handler's order: sizes mixed in one batch
        assert st[1] is True and st[2] == 3 * step                              # images=None, first_image_id
        for i in range(3):                                                      # the SOURCE boxes, mapped by the drawn record
            k = (3 * step + i) % 6
            src = np.asarray([[10.0, 20.0 + k, 70.0, 200.0]], np.float32)
            rec = {n: want[i][n] for n in want.dtype.names}
            wb, _ = ref_boxes(sizes[k & 1], (128, 416), True, rec, src, np.asarray([[1, 0, 0, 0]], np.float32), 0.25)
            assert st[3][i].tobytes() == wb.tobytes(), (step, i)


def test_augment_without_dataset_is_refused(stub_run):
    run_training, drawn = stub_run
    with pytest.raises(ValueError, match="--augment needs --dataset"):
        run_training.main(["--augment", "--steps", "1", "--no_resume"])
    assert drawn == [] and _StubEngine.log == []


def test_yaml_settings_reach_the_draw(stub_run, monkeypatch):
    run_training, drawn = stub_run
    from bayes_od_rc_amd import config_utils
    real = config_utils.load_yaml

    def with_settings(path):
        cfg = real(path)
        cfg["training_config"]["augmentation"] = {"flip_probability": 1.0, "min_visible": 0.5}
        return cfg
    monkeypatch.setattr(run_training.config_utils, "load_yaml", with_settings)
    run_training.main(["--dataset", "--augment", "--steps", "1", "--no_resume"])
    assert drawn[0][0]["flip_probability"] == 1.0 and drawn[0][0]["min_visible"] == 0.5 and drawn[0][0]["gain_range"] == [0.8, 1.2]
    assert _StubEngine.log[0][1]["flip"].all()


def test_kitti_handler_keeps_the_source_boxes(tmp_path):
    """The handler's ratio-scaled boxes are what they were; the source-pixel boxes ride beside them."""
    from PIL import Image
    from bayes_od_rc_amd import config_utils, constants, datasets, run_inference
    root = tmp_path / "object"
    (root / "training" / "image_2").mkdir(parents=True)
    (root / "training" / "label_2").mkdir()
    (root / "train.txt").write_text("000000\n")
    Image.fromarray(np.zeros((94, 310, 3), np.uint8)).save(str(root / "training" / "image_2" / "000000.png"))
    (root / "training" / "label_2" / "000000.txt").write_text("Car 0.00 0 -1.57 100.00 20.00 200.00 80.00 1.5 1.6 3.9 1.0 1.5 10.0 -1.5\n")
    here = os.path.dirname(os.path.abspath(run_inference.__file__))
    cfg = config_utils.load_yaml(os.path.join(here, "configs", "retinanet_bdd_covar.yaml"))["dataset_config"]
    cfg["dataset"] = "kitti"
    cfg["data_split"] = "train"
    cfg["kitti"]["paths_config"]["dataset_dir"] = str(root)
    cfg["kitti"]["resize_shape"] = [128, 416]
    handler = datasets.build_dataset(cfg, "train")
    handler.dense_targets = False
    sample = next(iter(handler.create_dataset()))
    src = np.asarray([[20.0, 100.0, 80.0, 200.0]], np.float32)
    assert np.array_equal(sample[datasets.BOXES_2D_GT_SOURCE_KEY], src)
    scaled = (src / np.array([94, 310, 94, 310], np.float32)) * np.array([128, 416, 128, 416], np.float32)
    assert np.array_equal(sample[constants.BOXES_2D_GT_KEY], scaled)


def test_the_three_entry_points_are_declared():
    import ctypes
    from bayes_od_rc_amd import _lib, build
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bayesod.h")).read(), flags=re.S)
    cdef = open(os.path.join(ROOT, "include", "bayesod_cdef.h")).read()
    for name in NAMES:
        assert re.search(r"\bbod_status\s+%s\s*\(" % name, header), name
        assert re.search(r"\bbod_status\s+%s\s*\(" % name, cdef), name
        assert name in _lib.SIGNATURES
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, header).group(1)
        assert len(args.split(",")) == len(_lib.SIGNATURES[name][1]), name
        assert getattr(_lib.load(), name) is not None
    assert "} bod_augment;" in header and "} bod_augment;" in cdef
    assert cdef == build.cdef_text()
    from bayes_od_rc_amd.engine import AUGMENT_DTYPE
    assert ctypes.sizeof(_lib.BodAugment) == AUGMENT_DTYPE.itemsize == 24
    assert [f[0] for f in _lib.BodAugment._fields_] == list(AUGMENT_DTYPE.names)
