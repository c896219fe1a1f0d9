"""Mergeable MC statistics on the GPU (include/bayesod.h, mc_statistics): the merge kernel against the float64 statement of its
formula, stat_from_raw_kernel against the fused epilogues, passes / handles / weight sets / ranks folded into ONE posterior
against the reference (oracle.bayes_od on the union of the samples), and default handles left as they were."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import ANCHOR_CFG, BAYES_CFG, NMS_CFG, ROOT, compare_posterior

pytestmark = pytest.mark.gpu
REL_TOL = 1e-3          # tests/test_gpu_post.py: the project's bar
HW, B = (128, 128), 2
SEED, FIRST = 20261018, 3


def _anchors(hw=HW):
    from bayes_od_rc_amd.anchor_generator import FpnAnchorGenerator
    return FpnAnchorGenerator(ANCHOR_CFG).generate_all((hw[0], hw[1], 3))


def _engine(n, batch=B, hw=HW, weights=True, weight_seed=1000, **kw):
    from bayes_od_rc_amd import synthetic
    from bayes_od_rc_amd.engine import Engine, make_config
    eng = Engine(make_config(hw, batch=batch, mc_samples=n, bayes_od_config=BAYES_CFG, nms_config=NMS_CFG, use_full_covar=True, **kw))
    if weights:
        eng.load_weights(synthetic.make_weights(cls_fg_bias=-1.0, seed=weight_seed))
        eng.set_anchors(_anchors(hw))
    return eng


def _frames(batch=B, hw=HW):
    from bayes_od_rc_amd import synthetic
    return synthetic.make_frames(batch, hw[0], hw[1], seed=31)


def _oracle(raw, anchors, img, seed=SEED, first=FIRST):
    """The reference on the union of the samples: raw = (cls, box, cov) [B,N,A,.] -- the device's own fp32 head outputs."""
    from oracle import bayes_od, network, philox
    cls, box, cov = raw
    u = philox.categorical_uniforms(seed, first + img, cls.shape[2])
    pred = {"anchors_class_predictions": cls[img], "anchors_box_predictions": box[img],
            "anchors_box_covar_predictions": network.fill_triangular_4(cov[img])}
    return bayes_od.bayes_od_posterior(pred, anchors, u, BAYES_CFG, use_full_covar=True, dtype=np.float64, return_debug=True), u


def _concat(raws):
    return tuple(np.concatenate([r[k] for r in raws], axis=1) for k in range(3))


def _check_against_oracle(eng, raws, anchors=None):
    anchors = _anchors() if anchors is None else anchors
    raw = _concat(raws)
    refs = []
    for img in range(eng.B):
        ref, u = _oracle(raw, anchors, img)
        n, _ = compare_posterior(eng.get_posterior(img), ref, u, tol=REL_TOL, min_checked=20)
        print("image %d: %d anchors compared with the oracle on %d samples" % (img, n, raw[0].shape[1]))
        refs.append((ref, u))
    return refs


# ------------------------------------------------------------------------------------------------ 1. the merge kernel alone
def _group_record(rng, n, ba):
    """fp32 statistics record of n random samples per anchor (float64 group statistics, rounded once)."""
    centre = rng.uniform(0.0, 128.0, (1, ba, 2))
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
    logits = rng.normal(0, 2.0, (n, ba, 8))
    p = np.exp(logits - logits.max(axis=2, keepdims=True))
    cls = (p / p.sum(axis=2, keepdims=True)).sum(axis=0)
    cov = rng.normal(0, 0.4, (n, ba, 10)).sum(axis=0)
    return cls.astype(np.float32), box.astype(np.float32), cov.astype(np.float32)


@pytest.mark.parametrize("batch", [2, 3])           # A = 3 069: no multiple of the block or of 4; B = 3: B*A*10 floats end in a partial float4
def test_merge_kernel_against_float64(batch):
    from bayes_od_rc_amd.distributed import merge_statistics_np
    dst = _engine(2, batch=batch, weights=False, mc_statistics=True)
    src = _engine(2, batch=batch, weights=False, mc_statistics=True)
    a_n = dst.A
    assert a_n == 3069 and a_n % 4 != 0 and a_n % 256 != 0
    shape = lambda rec: tuple(x.reshape(batch, a_n, -1) for x in rec)
    rng = np.random.default_rng(77 + batch)
    for ka, kb in ((1, 4), (5, 5), (2, 7), (0, 6)):
        rb = shape(_group_record(rng, kb, batch * a_n))
        if ka:
            ra = shape(_group_record(rng, ka, batch * a_n))
        else:
            ra = tuple(np.full_like(x, np.nan) for x in rb)          # an empty accumulator's contents are never read
        src.set_statistics(*rb, samples=kb)
        runs = []
        for via_pointers in (True, False, True):
            dst.set_statistics(*ra, samples=ka)
            if via_pointers:
                dst.stat_merge(src.stat_device_pointers(), kb)
            else:
                dst.stat_merge_from(src)
            runs.append(dst.get_statistics())
        for x, y in zip(src.get_statistics()[:3], rb):
            assert np.array_equal(x, y)                              # the source is left unchanged
        cls, box, cov, k = runs[0]
        assert k == ka + kb == dst.stat_samples
        for other in runs[1:]:                                       # the same bits again, through either entry point
            assert other[3] == k and all(np.array_equal(p, q) for p, q in zip(other[:3], (cls, box, cov)))
        assert np.all(box[..., 14:] == 0)
        if ka == 0:
            assert np.array_equal(cls, rb[0]) and np.array_equal(box, rb[1]) and np.array_equal(cov, rb[2])
            continue
        assert np.array_equal(cls, ra[0] + rb[0]) and np.array_equal(cov, ra[2] + rb[2])       # one fp32 rounding each
        ref = merge_statistics_np(ra, rb, ka, kb, dtype=np.float64)                           # of the SAME fp32 inputs
        a64, b64 = ra[1].astype(np.float64), rb[1].astype(np.float64)
        err = np.abs(box.astype(np.float64) - ref[1])
        mean_bound = 5e-7 * (np.abs(a64[..., :4]) + np.abs(b64[..., :4]))
        print("(%d, %d): mean error / bound %.3f" % (ka, kb, float((err[..., :4] / mean_bound).max())))
        assert np.all(err[..., :4] <= mean_bound)
        d = b64[..., :4] - a64[..., :4]
        k = 4
        worst = 0.0
        for i in range(4):
            for j in range(i + 1):
                bound = 1e-6 * (np.abs(a64[..., k]) + np.abs(b64[..., k]) + np.abs(d[..., i] * d[..., j]) * ka * kb / (ka + kb))
                worst = max(worst, float((err[..., k] / bound).max()))
                assert np.all(err[..., k] <= bound), (ka, kb, i, j)
                k += 1
        print("(%d, %d): M2 error / bound %.3f" % (ka, kb, worst))


# ------------------------------------------------------------------ 2. / 7. subprocess runs on the forced 256-row tile (aggregating plans)
_SCRIPT = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from conftest import ANCHOR_CFG, BAYES_CFG, NMS_CFG
from bayes_od_rc_amd import synthetic
from bayes_od_rc_amd.anchor_generator import FpnAnchorGenerator
from bayes_od_rc_amd.engine import Engine, make_config
precision, stat = sys.argv[3], sys.argv[4] == "stat"
h, w, batch, n = 128, 160, 2, 5
eng = Engine(make_config((h, w), batch=batch, mc_samples=n, bayes_od_config=BAYES_CFG, nms_config=NMS_CFG, use_full_covar=True,
                         precision=precision, mc_statistics=stat))
eng.load_weights(synthetic.make_weights(cls_fg_bias=-1.0))
eng.set_anchors(FpnAnchorGenerator(ANCHOR_CFG).generate_all((h, w, 3)))
frames = synthetic.make_frames(batch, h, w, seed=31)
info = eng.plan_info()
out = {"aggregating": np.int32(eng.aggregating), "sparse_tail": np.int32(info["sparse_tail"]), "sparse_halo": np.int32(info["sparse_halo"]),
       "ops": np.int32(info["ops"]), "anchors": np.int32(eng.A)}
out["device_bytes"] = np.int64(eng.device_bytes)       # (before anything asks for the lazily allocated raw tensors)
eng.infer(frames, seed=77, first_image_id=5)
for b in range(batch):
    for k, v in eng.get_posterior(b).items():
        out["post%d_%s" % (b, k)] = v
    for k, v in zip(("scores", "means", "covs", "counts"), eng.get_detections(b)):
        out["det%d_%s" % (b, k)] = v
if stat:
    assert eng.stat_samples == 0                      # infer / forward / posterior leave the accumulator alone
    eng.stat_forward(frames, seed=77, first_image_id=5, sample_base=5)
    cls, box, cov, k = eng.get_statistics()
    assert k == n
    out.update(stat_cls=cls, stat_box=box, stat_cov=cov)
    for name, a in zip(("cls", "box", "cov"), eng.get_raw()):          # the raw outputs of that very pass (samples 5 .. 9)
        out["raw_" + name] = a
np.savez(sys.argv[2], **out)
"""
_RUNS = {}


def _run(tmp_path_factory, precision, mode, **env):
    key = (precision, mode, tuple(sorted(env.items())))
    if key not in _RUNS:
        path = str(tmp_path_factory.mktemp("stat") / "out.npz")
        r = subprocess.run([sys.executable, "-c", _SCRIPT, ROOT, path, precision, mode],
                           env=dict(os.environ, BOD_FORCE_CONV_TILE="256", **env), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
        z = np.load(path)
        _RUNS[key] = {k: z[k] for k in z.files}
    return _RUNS[key]


@pytest.mark.parametrize("precision", ["bf16", "bf16x3"])
def test_stat_from_raw_equals_the_fused_epilogues(tmp_path_factory, precision):
    """(128,160), B = 2, n = 5 on the forced tile: the record of the aggregating flavour (fused epilogues) against the record
    stat_from_raw_kernel makes of a raw-flavour forward with the same seed and sample base (BOD_FUSE_AGGREGATION=0: no aggregating
    plan, so the same statistics handle takes the raw route) -- bit for bit."""
    fused = _run(tmp_path_factory, precision, "stat")
    raw = _run(tmp_path_factory, precision, "stat", BOD_FUSE_AGGREGATION="0")
    assert int(fused["aggregating"]) == 1 and int(raw["aggregating"]) == 0
    for k in ("raw_cls", "raw_box", "raw_cov"):
        assert np.array_equal(fused[k], raw[k]), k            # the same head outputs went into both reductions
    for k in ("stat_cls", "stat_box", "stat_cov"):
        assert np.array_equal(fused[k], raw[k]), k
    assert np.all(fused["stat_box"][..., 14:] == 0) and np.abs(fused["stat_box"][..., 4]).max() > 0


def test_default_handles_are_untouched(tmp_path_factory):
    plain = _run(tmp_path_factory, "bf16", "plain")
    dense = _run(tmp_path_factory, "bf16", "plain", BOD_SPARSE_TAIL="0")
    stat = _run(tmp_path_factory, "bf16", "stat")
    # the default handle still plans the sparse tail and its halo; a statistics handle's aggregating plan is the dense one
    assert (int(plain["aggregating"]), int(plain["sparse_tail"]), int(plain["sparse_halo"])) == (1, 1, 1)
    assert (int(dense["aggregating"]), int(dense["sparse_tail"]), int(dense["sparse_halo"])) == (1, 0, 0)
    assert (int(stat["aggregating"]), int(stat["sparse_tail"]), int(stat["sparse_halo"])) == (1, 0, 0)
    assert int(stat["ops"]) == int(dense["ops"])
    # device memory: the accumulator (34 floats per anchor and image) is the whole difference to the dense plain handle,
    # which therefore holds none; the default handle adds its sparse tables to that
    acc = 2 * int(stat["anchors"]) * (8 + 16 + 10) * 4
    assert int(stat["device_bytes"]) - int(dense["device_bytes"]) == acc
    assert int(plain["device_bytes"]) > int(dense["device_bytes"])
    # dense against dense: a statistics handle's infer is the plain handle's, bit for bit
    for k in dense:
        if k.startswith(("post", "det")):
            assert np.array_equal(stat[k], dense[k]), k
    assert dense["det0_means"].shape[0] > 0


def test_stat_calls_refuse_a_plain_handle():
    plain = _engine(2, weights=False)
    stat = _engine(2, weights=False, mc_statistics=True)
    z = np.zeros((B, plain.A, 8), np.float32), np.zeros((B, plain.A, 16), np.float32), np.zeros((B, plain.A, 10), np.float32)
    calls = [plain.stat_reset, lambda: plain.stat_forward(_frames()), lambda: plain.stat_merge_from(stat),
             lambda: plain.stat_merge(stat.stat_device_pointers(), 2), plain.stat_device_pointers, lambda: plain.stat_samples,
             plain.get_statistics, lambda: plain.set_statistics(*z, samples=2), plain.stat_posterior,
             lambda: stat.stat_merge_from(plain)]
    for call in calls:
        with pytest.raises(ValueError):
            call()
    # two handles without weights differ by the accumulator alone: 34 floats per anchor and image, reported in device_bytes
    assert stat.device_bytes - plain.device_bytes == B * plain.A * (8 + 16 + 10) * 4
    other = _engine(2, batch=3, weights=False, mc_statistics=True)
    with pytest.raises(ValueError, match="batch"):
        stat.stat_merge_from(other)
    with pytest.raises(ValueError):                     # stage order: weights and anchors first
        stat.stat_forward(_frames())


# ------------------------------------------------------------------------------------------------ 3. passes = one big handle = the reference
def test_two_passes_equal_the_reference_and_a_plain_handle():
    frames, anchors = _frames(), _anchors()
    eng = _engine(5, mc_statistics=True, mc_ensemble_size=10)
    raws = []
    for base in (0, 5):
        eng.stat_forward(frames, seed=SEED, first_image_id=FIRST, sample_base=base)
        raws.append(eng.get_raw())                      # the raw head outputs of that pass
    assert eng.stat_samples == 10
    eng.stat_posterior(seed=SEED, first_image_id=FIRST)
    refs = _check_against_oracle(eng, raws, anchors)                    # (a): the binding clause
    eng.nms()
    eng.cluster_fuse()
    assert all(np.isfinite(eng.get_detections(b)[2]).all() for b in range(B))

    # (b) a plain handle with mc_samples = 10 and the same seed: Welford re-association only
    plain = _engine(10)
    plain.forward(frames, seed=SEED, first_image_id=FIRST)
    plain.posterior(seed=SEED, first_image_id=FIRST)
    for img, (ref, u) in enumerate(refs):
        got, want = eng.get_posterior(img), plain.get_posterior(img)
        cdf = np.cumsum(ref["mean_probs"], axis=1)
        t = u.astype(np.float64) * cdf[:, -1:]
        ambiguous = np.abs(cdf[:, None, :] - t[:, :, None]).min(axis=(1, 2)) < 1e-5
        assert ambiguous.mean() < 5e-3
        gk, wk = np.zeros(eng.A, bool), np.zeros(eng.A, bool)
        gk[got["anchor_index"]] = True
        wk[want["anchor_index"]] = True
        assert not np.any((gk != wk) & ~ambiguous)
        both = np.nonzero(gk & wk & ~ambiguous)[0]
        assert len(both) >= 20
        gi, wi = np.searchsorted(got["anchor_index"], both), np.searchsorted(want["anchor_index"], both)
        assert np.array_equal(got["counts"][gi], want["counts"][wi])
        mean_err = np.max(np.abs(got["means"][gi] - want["means"][wi]) / (np.abs(want["means"][wi]) + 1.0))
        cw = want["covs"][wi]
        floor = np.abs(cw).reshape(len(cw), -1).max(axis=1)[:, None, None] * 1e-2
        cov_err = (np.abs(got["covs"][gi] - cw) / (np.abs(cw) + floor)).max()
        print("image %d: %d anchors against the plain handle, mean %.3g cov %.3g" % (img, len(both), mean_err, cov_err))
        assert mean_err < 1e-4 and cov_err < 5e-4        # test_fused_mc_aggregation_equals_the_raw_path's bounds


def test_uneven_passes_on_two_handles_equal_the_reference():
    """(c): n = 4 on one handle, n = 6 on a second one, folded with stat_merge_from."""
    frames = _frames()
    first = _engine(4, mc_statistics=True, mc_ensemble_size=10)
    second = _engine(6, mc_statistics=True, mc_ensemble_size=10)
    first.stat_forward(frames, seed=SEED, first_image_id=FIRST, sample_base=0)
    second.stat_forward(frames, seed=SEED, first_image_id=FIRST, sample_base=4)
    raws = [first.get_raw(), second.get_raw()]
    first.stat_merge_from(second)
    assert (first.stat_samples, second.stat_samples) == (10, 6)
    first.stat_posterior(seed=SEED, first_image_id=FIRST)
    _check_against_oracle(first, raws)
    first.stat_reset()
    assert first.stat_samples == 0
    with pytest.raises(ValueError):
        first.stat_posterior(seed=SEED, first_image_id=FIRST)


# ------------------------------------------------------------------------------------------------ 4. / 5. ensembles
def _model(weight_seed, n, dropout_rate=0.3):
    from bayes_od_rc_amd import synthetic
    from bayes_od_rc_amd.model import RetinaNetModel
    cfg = {"output_names": ["classification", "regression", "regression_covar"], "mc_dropout_samples": n,
           "header": {"dropout_rate": dropout_rate, "num_classes": 7, "anchors_per_location": 9}}
    model = RetinaNetModel(cfg)
    model.load_weights(synthetic.make_weights(cls_fg_bias=-1.0, seed=weight_seed))
    return model


def test_ensemble_of_two_weight_sets_equals_the_reference():
    from bayes_od_rc_amd.inference_utils import EnsemblePipeline
    frames, anchors = _frames(), _anchors()
    pipe = EnsemblePipeline([_model(1000, 3), _model(2000, 3)], HW, B, BAYES_CFG, NMS_CFG, 3, anchors=anchors)
    dets = pipe(frames, seed=SEED, first_image_id=FIRST)
    assert pipe.engine.stat_samples == 6 and len(dets) == B
    raws = [e.get_raw() for e in pipe.engines]          # member m drew samples 3m .. 3m + 2
    assert not np.array_equal(raws[0][0], raws[1][0])
    _check_against_oracle(pipe.engine, raws, anchors)
    for scores, means, covs, counts in dets:
        assert scores.shape[0] > 0 and scores.shape[1] == 8 and np.isfinite(covs).all()


def test_one_member_with_two_passes_equals_the_reference():
    from bayes_od_rc_amd.inference_utils import EnsemblePipeline
    frames, anchors = _frames(), _anchors()
    pipe = EnsemblePipeline([_model(1000, 3)], HW, B, BAYES_CFG, NMS_CFG, 3, passes=2, anchors=anchors)
    dets = pipe(frames, seed=SEED, first_image_id=FIRST)
    assert pipe.engine.stat_samples == 6
    last = pipe.engine.get_raw()                         # pass 1: samples 3 .. 5
    shard = _engine(3, mc_ensemble_size=6)               # the same samples from a plain handle of the sample-sharded kind
    raws = []
    for base in (0, 3):
        cfg = shard.cfg
        cfg.mc_sample_base = base
        shard.update_config(cfg)
        shard.forward(frames, seed=SEED, first_image_id=FIRST)
        raws.append(shard.get_raw())
    assert all(np.array_equal(a, b) for a, b in zip(raws[1], last))
    _check_against_oracle(pipe.engine, raws, anchors)
    assert all(d[0].shape[0] > 0 for d in dets)


def test_single_sample_members_take_the_raw_route():
    """Three members of n = 1 with dropout_rate = 0: no aggregating plan exists for one sample, so every record comes from
    stat_from_raw_kernel; and one sample alone gives no posterior."""
    from bayes_od_rc_amd.inference_utils import EnsemblePipeline
    frames, anchors = _frames(), _anchors()
    pipe = EnsemblePipeline([_model(s, 1, dropout_rate=0.0) for s in (1000, 2000, 3000)], HW, B, BAYES_CFG, NMS_CFG, 1, anchors=anchors)
    assert not any(e.aggregating for e in pipe.engines)
    dets = pipe(frames, seed=SEED, first_image_id=FIRST)
    assert pipe.engine.stat_samples == 3
    _check_against_oracle(pipe.engine, [e.get_raw() for e in pipe.engines], anchors)
    assert all(np.isfinite(d[2]).all() for d in dets)
    one = pipe.engines[1]
    one.stat_reset()
    one.stat_forward(frames, seed=SEED, first_image_id=FIRST, sample_base=0)
    assert one.stat_samples == 1
    with pytest.raises(ValueError, match="2"):
        one.stat_posterior(seed=SEED, first_image_id=FIRST)


# ------------------------------------------------------------------------------------------------ 6. two ranks on one GPU
def test_stat_sharded_two_ranks_on_one_gpu(tmp_path):
    """StatShardedEngine with N = 10 over two processes (both on this GPU, gloo): the detections are equal across the ranks bit
    for bit and the posterior meets the oracle on the union of the two ranks' raw samples (tests/tools/stat_shard_worker.py)."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    worker = os.path.join(ROOT, "tests", "tools", "stat_shard_worker.py")
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), LOCAL_RANK=str(rank))
        procs.append(subprocess.Popen([sys.executable, worker, str(tmp_path)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=300))      # each worker under its own limit
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for p, (so, se) in zip(procs, outs):
        assert p.returncode == 0, (so[-1500:], se[-3000:])
    assert "STAT_SHARD_OK" in outs[0][0], outs[0]
    a, b = np.load(str(tmp_path / "rank0.npz")), np.load(str(tmp_path / "rank1.npz"))
    assert sorted(a.files) == sorted(b.files) and len(a.files) >= 4
    for k in a.files:
        assert np.array_equal(a[k], b[k]), k
    assert a["det0_means"].shape[0] > 0
