"""Horizontal-flip views of the MC statistics on the GPU (include/bayesod.h, bod_stat_forward_view / bod_stat_merge_view): the
mirrored fold against distributed.mirror_statistics_np, a mirrored forward of mirrored frames against the plain forward, the
posterior of an identity pass and a mirrored pass against the NumPy merge of their records, device image buffers, the refusals and
EnsemblePipeline(views=...).  Everything but the second half of the kernel test is compared for equality."""
import ctypes

import numpy as np
import pytest

from conftest import ANCHOR_CFG, BAYES_CFG, NMS_CFG

pytestmark = pytest.mark.gpu
SEED, FIRST = 20261018, 3
# (128,128): level widths 16, 8, 4, 2, 1.  (64,384): widths 48 .. 3, not square, an odd top level, B*A*10 no multiple of 4.
SHAPES = {"square": ((128, 128), 2), "wide": ((64, 384), 3)}
K = 9
_ENGINES = {}


def _anchors(hw):
    from bayes_od_rc_amd.anchor_generator import FpnAnchorGenerator
    return FpnAnchorGenerator(ANCHOR_CFG).generate_all((hw[0], hw[1], 3))


def _engine(n, hw, batch, weights=True, anchors=True, classes=8, covar=True, cache=None, **kw):
    """A handle; ``cache``: a key under which the tests of this file share it (statistics handles are reset before use)."""
    from bayes_od_rc_amd import synthetic
    from bayes_od_rc_amd.engine import Engine, make_config
    if cache is not None and cache in _ENGINES:
        return _ENGINES[cache]
    eng = Engine(make_config(hw, batch=batch, mc_samples=n, bayes_od_config=BAYES_CFG, nms_config=NMS_CFG, use_full_covar=True,
                             num_classes=classes, has_covar_head=covar, **kw))
    if weights:
        eng.load_weights(synthetic.make_weights(cls_fg_bias=-1.0, seed=1000))
    if anchors:
        eng.set_anchors(_anchors(hw))
    if cache is not None:
        _ENGINES[cache] = eng
    return eng


def _frames(hw, batch):
    from bayes_od_rc_amd import synthetic
    return synthetic.make_frames(batch, hw[0], hw[1], seed=31)


def _mirror(eng, rec):
    from bayes_od_rc_amd.distributed import mirror_statistics_np
    return mirror_statistics_np(rec[0], rec[1], rec[2], eng.levels, K, eng.cfg.image_w)


def _equal(got, want):
    return all((g is None and w is None) or np.array_equal(g, w) for g, w in zip(got[:3], want[:3]))


# ------------------------------------------------------------------------------------------------ a. the mirrored fold alone
def _group_record(rng, n, ba, hw, classes, covar):
    """fp32 statistics record of n random samples per anchor (float64 group statistics, rounded once)."""
    centre = np.concatenate([rng.uniform(0.0, hw[0], (1, ba, 1)), rng.uniform(0.0, hw[1], (1, ba, 1))], axis=2)
    size = rng.uniform(8.0, 90.0, (1, ba, 2))
    x = np.concatenate([centre, size], axis=2) + rng.normal(0.0, 1.5, (n, ba, 4))
    mean = x.mean(axis=0)
    d = x - mean
    m2 = np.einsum("nai,naj->aij", d, d)
    box = np.zeros((ba, 16))
    box[:, :4] = mean
    k = 4
    for i in range(4):
        for j in range(i + 1):
            box[:, k] = m2[:, i, j]
            k += 1
    logits = rng.normal(0, 2.0, (n, ba, classes))
    p = np.exp(logits - logits.max(axis=2, keepdims=True))
    cls = (p / p.sum(axis=2, keepdims=True)).sum(axis=0)
    cov = rng.normal(0, 0.4, (n, ba, 10)).sum(axis=0).astype(np.float32) if covar else None
    return cls.astype(np.float32), box.astype(np.float32), cov


@pytest.mark.parametrize("classes,covar", [(8, True), (4, False)])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_mirrored_fold_equals_mirror_statistics_np(shape, classes, covar):
    from bayes_od_rc_amd.distributed import merge_statistics_np
    hw, batch = SHAPES[shape]
    x = _engine(2, hw, batch, weights=False, classes=classes, covar=covar, mc_statistics=True)
    y = _engine(2, hw, batch, weights=False, classes=classes, covar=covar, mc_statistics=True)
    a_n = x.A
    if shape == "wide":
        assert [w for _, w in x.levels] == [48, 24, 12, 6, 3] and (batch * a_n * 10) % 4 != 0
    else:
        assert [w for _, w in x.levels] == [16, 8, 4, 2, 1]
    shaped = lambda rec: tuple(None if v is None else v.reshape(batch, a_n, -1) for v in rec)
    rng = np.random.default_rng(91 + classes)
    first = shaped(_group_record(rng, 3, batch * a_n, hw, classes, covar))
    second = shaped(_group_record(rng, 5, batch * a_n, hw, classes, covar))
    x.set_statistics(*first, samples=3)
    want = _mirror(x, first)
    assert not np.array_equal(want[1], first[1])
    # an empty accumulator: the result is the mirror map of the record, exactly
    y.stat_merge(x.stat_device_pointers(), 3, view="hflip")
    got = y.get_statistics()
    assert got[3] == 3 and _equal(got, want)
    assert _equal(x.get_statistics(), first)                             # the source is left unchanged
    # an accumulator of 5 samples: merge(second, mirror(first)); test_merge_kernel_against_float64's rule and bounds
    ka, kb = 5, 3
    y.set_statistics(*second, samples=ka)
    y.stat_merge(x.stat_device_pointers(), kb, view=1)
    cls, box, cov, k = y.get_statistics()
    assert k == ka + kb == y.stat_samples
    ra, rb = second, want
    assert np.all(box[..., 14:] == 0)
    assert np.array_equal(cls, ra[0] + rb[0]) and (not covar or np.array_equal(cov, ra[2] + rb[2]))       # one fp32 rounding each
    ref = merge_statistics_np(ra, rb, ka, kb, dtype=np.float64)                                          # of the SAME fp32 inputs
    a64, b64 = ra[1].astype(np.float64), rb[1].astype(np.float64)
    err = np.abs(box.astype(np.float64) - ref[1])
    mean_bound = 5e-7 * (np.abs(a64[..., :4]) + np.abs(b64[..., :4]))
    print("mean error / bound %.3f" % float((err[..., :4] / mean_bound).max()))
    assert np.all(err[..., :4] <= mean_bound)
    d = b64[..., :4] - a64[..., :4]
    k, worst = 4, 0.0
    for i in range(4):
        for j in range(i + 1):
            bound = 1e-6 * (np.abs(a64[..., k]) + np.abs(b64[..., k]) + np.abs(d[..., i] * d[..., j]) * ka * kb / (ka + kb))
            worst = max(worst, float((err[..., k] / bound).max()))
            assert np.all(err[..., k] <= bound), (i, j)
            k += 1
    print("M2 error / bound %.3f" % worst)


# ------------------------------------------------------------------------------------------------ b. view 0
def test_view_zero_is_stat_forward():
    hw, batch = SHAPES["square"]
    eng = _engine(3, hw, batch, mc_statistics=True, mc_ensemble_size=12, cache="square3")
    frames = _frames(hw, batch)
    eng.stat_reset()
    eng.stat_forward(frames, seed=SEED, first_image_id=FIRST, sample_base=3)
    want = eng.get_statistics()
    eng.stat_reset()
    eng.stat_forward(frames, seed=SEED, first_image_id=FIRST, sample_base=3, view="identity")
    assert _equal(eng.get_statistics(), want)
    eng.stat_reset()                                 # the new entry point itself with BOD_VIEW_IDENTITY
    eng._chk(eng.lib.bod_stat_forward_view(eng.h, frames.ctypes.data, 0, SEED, FIRST, 3, 0))
    got = eng.get_statistics()
    assert got[3] == 3 and _equal(got, want)
    ptrs = (ctypes.c_void_p * 3)(*eng.stat_device_pointers())
    other = _engine(3, hw, batch, weights=False, mc_statistics=True)
    other._chk(other.lib.bod_stat_merge_view(other.h, ptrs, 3, 0))
    assert _equal(other.get_statistics(), want)


# ------------------------------------------------------------------------------------------------ c. end to end
@pytest.mark.parametrize("n", [3, 1])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_mirrored_forward_of_mirrored_frames_is_the_mirror_of_the_forward(shape, n):
    """The library mirrors Fm = F[:, :, ::-1] back to F, so the record in front of the fold is the plain forward's; the
    accumulator is therefore mirror_statistics_np of the plain handle's, bit for bit.  n = 1 takes the raw route."""
    hw, batch = SHAPES[shape]
    plain = _engine(n, hw, batch, mc_statistics=True, mc_ensemble_size=12, cache=(shape, n, "a"))
    mirrored = _engine(n, hw, batch, mc_statistics=True, mc_ensemble_size=12, cache=(shape, n, "b"))
    frames = _frames(hw, batch)
    fm = np.ascontiguousarray(frames[:, :, ::-1, :])
    plain.stat_reset()
    mirrored.stat_reset()
    plain.stat_forward(frames, seed=SEED, first_image_id=FIRST, sample_base=5)
    mirrored.stat_forward(fm, seed=SEED, first_image_id=FIRST, sample_base=5, view="hflip")
    rec, got = plain.get_statistics(), mirrored.get_statistics()
    print("%s n=%d: aggregating plan %d" % (shape, n, int(plain.aggregating)))
    assert got[3] == n and (n == 1 or np.abs(rec[1][..., 5]).max() > 0)
    assert _equal(got, _mirror(plain, rec))
    assert not np.array_equal(got[1], rec[1])


_AGG_SCRIPT = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_stat_mirror as t
hw, batch = t.SHAPES["square"]
frames = t._frames(hw, batch)
plain = t._engine(3, hw, batch, mc_statistics=True, mc_ensemble_size=12)
mirrored = t._engine(3, hw, batch, mc_statistics=True, mc_ensemble_size=12)
plain.stat_forward(frames, seed=t.SEED, first_image_id=t.FIRST, sample_base=5)
mirrored.stat_forward(np.ascontiguousarray(frames[:, :, ::-1, :]), seed=t.SEED, first_image_id=t.FIRST, sample_base=5, view="hflip")
rec, got = plain.get_statistics(), mirrored.get_statistics()
np.savez(sys.argv[2], aggregating=np.int32(plain.aggregating and mirrored.aggregating), levels=np.asarray(plain.levels),
         rec_cls=rec[0], rec_box=rec[1], rec_cov=rec[2], got_cls=got[0], got_box=got[1], got_cov=got[2], k=np.int32(got[3]))
"""


def test_mirrored_forward_on_the_aggregating_plan(tmp_path):
    """The same on the forced 256-row tile (a process-wide switch, hence the child process), where the plan of (128,128), n = 3
    reduces the samples inside the last tower layers' epilogues: the mirrored fold reads the fused epilogues' record."""
    import os
    import subprocess
    import sys
    from conftest import ROOT
    from bayes_od_rc_amd.distributed import mirror_statistics_np
    path = str(tmp_path / "out.npz")
    r = subprocess.run([sys.executable, "-c", _AGG_SCRIPT, ROOT, path], env=dict(os.environ, BOD_FORCE_CONV_TILE="256"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    z = np.load(path)
    assert int(z["aggregating"]) == 1 and int(z["k"]) == 3
    want = mirror_statistics_np(z["rec_cls"], z["rec_box"], z["rec_cov"], [tuple(l) for l in z["levels"]], K, SHAPES["square"][0][1])
    assert np.abs(z["rec_box"][..., 5]).max() > 0
    assert _equal((z["got_cls"], z["got_box"], z["got_cov"]), want)


# ------------------------------------------------------------------------------------------------ d. posterior
def test_identity_and_mirrored_pass_give_the_posterior_of_the_numpy_merge():
    from bayes_od_rc_amd.distributed import merge_statistics_np
    hw, batch = SHAPES["square"]
    n = 5
    eng = _engine(n, hw, batch, mc_statistics=True, mc_ensemble_size=10)
    frames = _frames(hw, batch)
    # the mirrored pass's record without the library's mirror: a plain forward of frames mirrored in NumPy, mapped back in NumPy
    eng.stat_forward(np.ascontiguousarray(frames[:, :, ::-1, :]), seed=SEED, first_image_id=FIRST, sample_base=n)
    second = _mirror(eng, eng.get_statistics())
    eng.stat_reset()
    eng.stat_forward(frames, seed=SEED, first_image_id=FIRST, sample_base=0)
    first = eng.get_statistics()[:3]
    eng.stat_forward(frames, seed=SEED, first_image_id=FIRST, sample_base=n, view="hflip")
    assert eng.stat_samples == 2 * n
    merged = merge_statistics_np(first, second, n, n, dtype=np.float32)
    assert _equal(eng.get_statistics(), merged)
    ref = _engine(n, hw, batch, weights=False, mc_statistics=True, mc_ensemble_size=10)
    ref.set_statistics(*merged, samples=2 * n)
    for e in (eng, ref):
        e.stat_posterior(seed=SEED, first_image_id=FIRST)
        e.nms()
        e.cluster_fuse()
    for img in range(batch):
        got, want = eng.get_posterior(img), ref.get_posterior(img)
        assert sorted(got) == sorted(want) and len(got["anchor_index"]) > 0
        for key in want:
            assert np.array_equal(got[key], want[key]), key
        dg, dw = eng.get_detections(img), ref.get_detections(img)
        assert dw[0].shape[0] >= 1                   # at least one detection in every image
        assert all(np.array_equal(g, w) for g, w in zip(dg, dw))


# ------------------------------------------------------------------------------------------------ e. device buffers
def test_mirrored_forward_reads_the_device_buffer_and_leaves_it_alone():
    hw, batch = SHAPES["square"]
    eng = _engine(3, hw, batch, mc_statistics=True, mc_ensemble_size=12, cache="square3")
    frames = _frames(hw, batch)
    runs = {}

    def run(key, images, **kw):
        eng.stat_reset()
        eng.stat_forward(images, seed=SEED, first_image_id=FIRST, sample_base=3, **kw)
        runs[key] = eng.get_statistics()
    run("host_flip", frames, view="hflip")
    eng.upload_images(frames)
    run("dev_id_before", None)
    run("dev_flip", None, view="hflip")
    run("dev_id_after", None)
    assert np.array_equal(eng.get_images(), frames)                      # the source buffer is not modified
    assert _equal(runs["dev_flip"], runs["host_flip"])
    assert _equal(runs["dev_id_after"], runs["dev_id_before"])
    assert not _equal(runs["dev_flip"], runs["dev_id_before"])


# ------------------------------------------------------------------------------------------------ f. refusals
def test_view_refusals_leave_the_accumulator_alone():
    hw, batch = SHAPES["square"]
    frames = _frames(hw, batch)
    eng = _engine(3, hw, batch, mc_statistics=True, mc_ensemble_size=12, cache="square3")
    eng.stat_reset()
    eng.stat_forward(frames, seed=SEED, first_image_id=FIRST, sample_base=0)
    before = eng.get_statistics()
    src = _engine(2, hw, batch, weights=False, mc_statistics=True)
    ptrs = src.stat_device_pointers()
    for call in (lambda: eng.stat_forward(frames, sample_base=3, view=2), lambda: eng.stat_merge(ptrs, 2, view=2),
                 lambda: eng.stat_merge(ptrs, 2, view=-1), lambda: eng.stat_forward(frames, sample_base=3, view="vflip"),
                 lambda: eng.stat_forward(frames, sample_base=11, view="hflip")):          # (base 11 + 3 samples > 12)
        with pytest.raises(ValueError):
            call()
        assert eng.stat_samples == 3
    assert _equal(eng.get_statistics(), before)
    # (128,160): level 6 has 3 columns at 32, 96, 160 of a 160-pixel frame
    odd = _engine(2, (128, 160), batch, mc_statistics=True)
    odd.stat_forward(_frames((128, 160), batch), seed=SEED, first_image_id=FIRST)
    own = _engine(2, (128, 160), batch, weights=False, mc_statistics=True).stat_device_pointers()
    for call in (lambda: odd.stat_forward(_frames((128, 160), batch), view="hflip"), lambda: odd.stat_merge(own, 2, view="hflip")):
        with pytest.raises(ValueError, match="level 6"):
            call()
        assert odd.stat_samples == 2
    # a plain handle; a statistics handle without anchors
    plain = _engine(2, hw, batch, weights=False)
    for call in (lambda: plain.stat_forward(frames, view="hflip"), lambda: plain.stat_merge(ptrs, 2, view="hflip")):
        with pytest.raises(ValueError, match="mc_statistics"):
            call()
    bare = _engine(2, hw, batch, weights=False, anchors=False, mc_statistics=True)
    z = np.zeros((batch, bare.A, 8), np.float32), np.zeros((batch, bare.A, 16), np.float32), np.zeros((batch, bare.A, 10), np.float32)
    bare.set_statistics(*z, samples=4)
    with pytest.raises(ValueError, match="bod_set_anchors"):
        bare.stat_merge(ptrs, 2, view="hflip")
    assert bare.stat_samples == 4
    bare.stat_merge(ptrs, 2)                          # view 0 needs none
    assert bare.stat_samples == 6
    bare.set_anchors(_anchors(hw))
    bare.stat_merge(ptrs, 2, view="hflip")
    assert bare.stat_samples == 8


# ------------------------------------------------------------------------------------------------ g. EnsemblePipeline
def _model(weight_seed, n):
    from bayes_od_rc_amd import synthetic
    from bayes_od_rc_amd.model import RetinaNetModel
    cfg = {"output_names": ["classification", "regression", "regression_covar"], "mc_dropout_samples": n,
           "header": {"dropout_rate": 0.3, "num_classes": 7, "anchors_per_location": 9}}
    model = RetinaNetModel(cfg)
    model.load_weights(synthetic.make_weights(cls_fg_bias=-1.0, seed=weight_seed))
    return model


def test_ensemble_pipeline_views():
    from bayes_od_rc_amd.inference_utils import EnsemblePipeline
    hw, batch = SHAPES["square"]
    frames, anchors, n = _frames(hw, batch), _anchors(hw), 2
    models = [_model(1000, n), _model(2000, n)]
    pipe = EnsemblePipeline(models, hw, batch, BAYES_CFG, NMS_CFG, n, passes=2, anchors=anchors, views=("identity", "hflip"))
    assert pipe.total == 2 * 2 * 2 * n and pipe.engine.cfg.mc_ensemble_size == pipe.total
    dets = pipe(frames, seed=SEED, first_image_id=FIRST)
    assert pipe.engine.stat_samples == pipe.total
    got = pipe.engine.get_statistics()
    # the manual sequence: member m, pass p, view v draws the samples ((m * passes + p) * V + v) * n ..
    for m, eng in enumerate(pipe.engines):
        eng.stat_reset()
        for p in range(2):
            for v, view in enumerate((0, 1)):
                eng.stat_forward(frames, seed=SEED, first_image_id=FIRST, sample_base=((m * 2 + p) * 2 + v) * n, view=view)
    pipe.engine.stat_merge_from(pipe.engines[1])
    assert _equal(pipe.engine.get_statistics(), got)
    pipe.engine.stat_posterior(seed=SEED, first_image_id=FIRST)
    pipe.engine.nms()
    pipe.engine.cluster_fuse()
    for b in range(batch):
        assert dets[b][0].shape[0] > 0 and all(np.array_equal(g, w) for g, w in zip(pipe.engine.get_detections(b), dets[b]))
    # the uploaded batch: with images=None every view of every member reads member 0's buffer
    pipe.engine.upload_images(frames)
    again = pipe(None, seed=SEED, first_image_id=FIRST)
    assert all(np.array_equal(g, w) for b in range(batch) for g, w in zip(again[b], dets[b]))

    # without `views`: today's sample bases, ensemble size and bits
    today = EnsemblePipeline(models, hw, batch, BAYES_CFG, NMS_CFG, n, passes=2, anchors=anchors)
    assert today.total == 2 * 2 * n and today.engine.cfg.mc_ensemble_size == today.total and today.views == [0]
    dets = today(frames, seed=SEED, first_image_id=FIRST)
    got = today.engine.get_statistics()
    for m, eng in enumerate(today.engines):
        eng.stat_reset()
        for p in range(2):
            eng._chk(eng.lib.bod_stat_forward(eng.h, frames.ctypes.data, 0, SEED, FIRST, (m * 2 + p) * n))
    today.engine.stat_merge_from(today.engines[1])
    assert _equal(today.engine.get_statistics(), got)
    explicit = EnsemblePipeline(models, hw, batch, BAYES_CFG, NMS_CFG, n, passes=2, anchors=anchors, views=("identity",))
    same = explicit(frames, seed=SEED, first_image_id=FIRST)
    assert all(np.array_equal(g, w) for b in range(batch) for g, w in zip(same[b], dets[b]))


# ------------------------------------------------------------------------------------------------ run_inference --tta_flip
def test_run_inference_tta_flip(tmp_path, monkeypatch):
    """--tta_flip alone is a one-member EnsemblePipeline of the yaml's checkpoint with two views (one per batch size: 3 frames at
    --batch 2 leave a tail of one); every frame is written; without the flag no such pipeline is made; a geometry without mirror
    partners exits with the library's message."""
    import os
    from bayes_od_rc_amd import inference_utils, run_inference
    made = []

    class Spy(inference_utils.EnsemblePipeline):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)
    monkeypatch.setattr(inference_utils, "EnsemblePipeline", Spy)
    monkeypatch.setenv("BAYESOD_DATA_DIR", str(tmp_path / "tta"))
    args = ["--gpu_device", "0", "--data_split", "test", "--synthetic", "3", "--batch", "2"]
    root = run_inference.main(args + ["--image_size", "128", "128", "--tta_flip"])
    for i in range(3):
        mean = np.load(os.path.join(root, "mean", "%06d.npy" % i))
        assert mean.ndim == 2 and mean.shape[1] == 4
    assert sorted(p.engine.B for p in made) == [1, 2]
    for p in made:
        assert len(p.models) == 1 and p.views == [0, 1] and p.passes == 1 and p.total == 2 * p.n == p.engine.stat_samples
    del made[:]
    monkeypatch.setenv("BAYESOD_DATA_DIR", str(tmp_path / "plain"))
    run_inference.main(args + ["--image_size", "128", "128"])
    assert not made
    with pytest.raises(SystemExit, match="level 6"):
        run_inference.main(args + ["--image_size", "128", "160", "--tta_flip"])
