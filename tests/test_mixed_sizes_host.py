"""CPU: the host side of batches of mixed source sizes -- packing for the ragged uploads, the unbucketed minibatch former of
run_training, the dataset-order route of run_validation with a fake engine, and the declarations of the two entry points."""
import os
import re

import numpy as np
import pytest

from conftest import ANCHOR_CFG, ROOT
from test_validation_boxes_host import _FakeEngine, _FakeModel, _samples

NAMES = ("bod_upload_frames_u8_ragged", "bod_upload_frames_u8_ragged_async")
SIZES = [(94, 310), (92, 306), (60, 300)]


def _frames(sizes, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, size=hw + (3,), dtype=np.uint8) for hw in sizes]


def test_pack_ragged_offsets_and_order():
    from bayes_od_rc_amd.engine import pack_ragged
    frames = _frames(SIZES)
    buf, sizes = pack_ragged(frames)
    assert buf.dtype == np.uint8 and buf.ndim == 1 and buf.flags["C_CONTIGUOUS"]
    assert sizes.dtype == np.int32 and sizes.tolist() == [list(hw) for hw in SIZES]
    offsets = [0, 3 * 94 * 310, 3 * (94 * 310 + 92 * 306)]
    assert buf.size == offsets[2] + 3 * 60 * 300
    for f, off in zip(frames, offsets):
        assert np.array_equal(buf[off:off + f.size].reshape(f.shape), f)
    # non-contiguous views are packed by value
    view = frames[0][::-1]
    buf2, _ = pack_ragged([view, frames[1], frames[2]], batch=3)
    assert np.array_equal(buf2[:view.size].reshape(view.shape), view) and np.array_equal(buf2[view.size:], buf[view.size:])


def test_pack_ragged_refusals():
    from bayes_od_rc_amd.engine import pack_ragged
    frames = _frames(SIZES)
    with pytest.raises(ValueError, match="expected 2 frames, got 3"):
        pack_ragged(frames, batch=2)
    with pytest.raises(ValueError, match="expected 4 frames"):
        pack_ragged(frames, batch=4)
    with pytest.raises(ValueError, match="frame 1"):
        pack_ragged([frames[0], frames[1].astype(np.float32), frames[2]])
    with pytest.raises(ValueError, match="frame 2"):
        pack_ragged([frames[0], frames[1], frames[2][:, :, :2]])
    with pytest.raises(ValueError, match="frame 0"):
        pack_ragged([frames[0][None], frames[1], frames[2]])
    with pytest.raises(ValueError, match="frame 1"):
        pack_ragged([frames[0], frames[1][:0], frames[2]])
    with pytest.raises(ValueError):
        pack_ragged([])


def _sized(sizes):
    from bayes_od_rc_amd import constants
    return [{constants.ORIGINAL_IM_SIZE_KEY: np.asarray([h, w, 3], np.int32), "tag": i} for i, (h, w) in enumerate(sizes)]


def test_ordered_minibatches_keep_dataset_order_and_carry_the_tail():
    from bayes_od_rc_amd.run_training import bucket_minibatches, ordered_minibatches
    a, b = (370, 1224), (375, 1242)
    sizes = [a, b, a, b, a, a, b]
    carry = []
    epoch1 = list(ordered_minibatches(iter(_sized(sizes)), 3, carry))
    assert [[s["tag"] for s in mb] for mb in epoch1] == [[0, 1, 2], [3, 4, 5]]
    assert [s["tag"] for s in carry] == [6]
    # the partial tail opens the first minibatch of the next epoch: no frame is dropped
    epoch2 = list(ordered_minibatches(iter(_sized(sizes)), 3, carry))
    assert [[s["tag"] for s in mb] for mb in epoch2] == [[6, 0, 1], [2, 3, 4]]
    assert [s["tag"] for s in carry] == [5, 6]
    # ... where the bucketed former reorders the same stream by size
    bucketed = list(bucket_minibatches(iter(_sized(sizes)), 3, {}))
    assert [[s["tag"] for s in mb] for mb in bucketed] == [[0, 2, 4], [1, 3, 6]]


def test_stream_minibatches_in_the_handlers_order():
    from bayes_od_rc_amd.run_training import stream_minibatches
    a, b = (370, 1224), (375, 1242)

    class Handler(object):
        def create_dataset(self):
            return iter(_sized([a, b, a, b, b]))
    stream = stream_minibatches(Handler(), 2, mixed_sizes=True)
    got = [[s["tag"] for s in next(stream)] for _ in range(5)]
    assert got == [[0, 1], [2, 3], [4, 0], [1, 2], [3, 4]]
    stream = stream_minibatches(Handler(), 2)                    # default: bucketed, as before
    assert [[s["tag"] for s in next(stream)] for _ in range(2)] == [[0, 2], [1, 3]]


class _RaggedFakeEngine(_FakeEngine):
    def upload_frames_u8(self, *a, **k):
        raise AssertionError("the mixed route uploads ragged")

    def upload_frames_u8_ragged(self, frames, means, aspect_resize=True):
        assert isinstance(frames, list) and len(frames) == self.B and all(f.dtype == np.uint8 and f.ndim == 3 for f in frames)
        self.tags = [int(f[0, 0, 0]) for f in frames]
        self.log.append(("upload", self.B, tuple(f.shape[:2] for f in frames), bool(aspect_resize)))


class _RaggedFakeModel(_FakeModel):
    def engine_for(self, hw, batch=None, mc_samples=None, **kw):
        from bayes_od_rc_amd.run_validation import VALIDATION_NMS
        assert mc_samples == 1 and kw == {"nms_config": VALIDATION_NMS}
        return self.engines.setdefault((tuple(hw), batch), _RaggedFakeEngine(batch, self.log))


def test_mixed_validation_route_runs_in_dataset_order(tmp_path):
    from bayes_od_rc_amd import constants, run_validation
    a, b = (32, 96), (30, 90)
    sizes = [a, b, a, a, b, a, b, a]
    config = {"dataset_config": {"dataset": "kitti", "anchor_generator": ANCHOR_CFG, "im_normalization": "Kitti",
                                 "kitti": {"resize_shape": [64, 128]}},
              "model_config": {"losses": {"loss_names": ["classification", "regression_covar"], "loss_weights": [5.0, 1.0]}}}
    samples = _samples([(64, 128)] * len(sizes))
    for s, hw in zip(samples, sizes):
        s[constants.IMAGE_NORMALIZED_KEY] = None
        s["image_uint8"] = np.full(hw + (3,), s["image_uint8"][0, 0, 0], np.uint8)
        s[constants.ORIGINAL_IM_SIZE_KEY] = np.asarray(hw + (3,), np.int32)
    log = []
    ids = ["%06d" % i for i in range(len(sizes))]
    model = _RaggedFakeModel(log)
    records, totals, sums, ndet = run_validation._validate_mixed(model, config, iter(samples), ids, str(tmp_path), None, 3)
    # one pass in dataset order, one tail batch, no buckets: two handles (batch 3 and the tail of 2) of the network size
    assert [e[1] for e in log if e[0] == "validate"] == [(0, 1, 2), (3, 4, 5), (6, 7)]
    assert [e[1:] for e in log if e[0] == "upload"] == [(3, (a, b, a), True), (3, (a, b, a), True), (2, (b, a), True)]
    assert sorted(model.engines) == [((64, 128), 2), ((64, 128), 3)]
    # totals in dataset order, from each frame's own sums (n_pos = 2) plus the regularisation term
    assert totals == [5.0 * 10.0 * (i + 1) / 2.0 + (2.0 + 1.0) / 2.0 + 0.25 for i in range(len(sizes))]
    assert abs(sums["regularization_loss"] - 0.25 * len(sizes)) < 1e-12
    assert records == [] and ndet == sum(i + 1 for i in range(len(sizes)))
    assert sorted(os.listdir(str(tmp_path))) == [i + ".txt" for i in ids]
    # every frame's corners are rescaled on the host by its OWN original size
    out = run_validation.validate_batch(model, config, samples[:3], mixed_sizes=True)
    n = np.asarray([64, 128] * 2, np.float32)
    for j, hw in enumerate(sizes[:3]):
        assert np.array_equal(out[j][3], (np.full((j + 1, 4), float(j), np.float32) / n) * np.asarray(hw * 2, np.float32))
    # the BDD form returns records in dataset order
    config["dataset_config"]["dataset"] = "bdd"
    bdd = _samples([(64, 64)] * 5)
    ids = ["f%d.jpg" % i for i in range(5)]
    records, totals, _, ndet = run_validation._validate_mixed(_RaggedFakeModel([]), config, iter(bdd), ids, None, ["car"] * 7, 2)
    assert [r["name"] for r in records] == [ids[i] for i in range(5) for _ in range(i + 1)] and ndet == len(records) == 15
    assert len(totals) == 5


def test_the_flag_reaches_the_routes(monkeypatch, tmp_path):
    from bayes_od_rc_amd import run_inference, run_training, run_validation
    import inspect
    monkeypatch.setenv("BAYESOD_DATA_DIR", str(tmp_path))
    assert inspect.signature(run_validation.validate_checkpoint).parameters["mixed_sizes"].default is False
    assert inspect.signature(run_validation.validate).parameters["mixed_sizes"].default is False
    seen = {}

    def fake_validate(config, samples, sample_ids, **kw):
        seen.update(kw)
        return []
    monkeypatch.setattr(run_validation, "validate", fake_validate)
    import bayes_od_rc_amd.run_training as rt
    monkeypatch.setattr(rt, "synthetic_samples", lambda n, *a, **k: [{}] * n)
    assert run_validation.main(["--synthetic", "2"]) == [] and seen["mixed_sizes"] is False
    assert run_validation.main(["--synthetic", "2", "--mixed_sizes"]) == [] and seen["mixed_sizes"] is False     # only with --dataset
    for mod in (run_inference, run_training, run_validation):
        assert "--mixed_sizes" in inspect.getsource(mod.main)


def test_the_two_entry_points_are_declared():
    from bayes_od_rc_amd import _lib, build
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bayesod.h")).read(), flags=re.S)
    cdef = open(os.path.join(ROOT, "include", "bayesod_cdef.h")).read()
    for name in NAMES:
        assert re.search(r"\bbod_status\s+%s\s*\(" % name, header), name
        assert re.search(r"\bbod_status\s+%s\s*\(" % name, cdef), name
        assert name in _lib.SIGNATURES
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, header).group(1)
        assert len(args.split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert cdef == build.cdef_text()                        # the generated file follows the header
