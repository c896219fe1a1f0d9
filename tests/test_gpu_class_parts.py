"""GPU tests of the class-entropy parts (bod_config.covariance_parts bit BOD_PARTS_CLASS): the entropy of every
posterior row's and every detection's MC class distribution split into aleatoric, epistemic (mutual information) and spatial
parts.

Float64 reference: tests/class_parts_reference.py on the raw logits and on oracle.bayes_od's debug output.  Bound: absolute
difference <= 1e-5 on every value.  The values are entropies of at most ln 8 = 2.08; an fp32 NumPy emulation of the formulas on
these inputs differs from float64 by at most 3.7e-7, which leaves about 25x for the device's expf / logf.  Frame sizes as
tests/test_gpu_cov_parts.py: 128 x 128 (A = 3 069), batch 2, N = 5, C = 8, and KITTI 96 x 160 for C = 4."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import class_parts_reference as clr
import post_reference
from conftest import ANCHOR_CFG, BAYES_CFG, NMS_CFG
from test_gpu_cov_parts import _rows_to_compare

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 1e-5
HW, BATCH, N = (128, 128), 2, 5
KITTI_HW, KITTI_ORIG = (96, 160), (375, 1242)
SEED, FIRST = 987654321987, 11
_cache = {}


def _anchors(hw):
    from bayes_od_rc_amd.anchor_generator import FpnAnchorGenerator
    if ("anchors", hw) not in _cache:
        _cache[("anchors", hw)] = FpnAnchorGenerator(ANCHOR_CFG).generate_all((hw[0], hw[1], 3))
    return _cache[("anchors", hw)]


def _engine(hw=HW, batch=BATCH, n=N, weights=False, bits=2, **kw):
    from bayes_od_rc_amd import synthetic
    from bayes_od_rc_amd.engine import Engine, make_config
    kw.setdefault("bayes_od_config", BAYES_CFG)
    kw.setdefault("nms_config", NMS_CFG)
    kw.setdefault("use_full_covar", True)
    eng = Engine(make_config(hw, batch=batch, mc_samples=n, covariance_parts=bool(bits & 1), class_parts=bool(bits & 2), **kw))
    assert eng.cfg.covariance_parts == bits
    if weights:
        eng.load_weights(synthetic.make_weights(cls_fg_bias=-1.0))
    eng.set_anchors(_anchors(hw))
    return eng


def _raw(hw, c=8):
    """The posterior tests' random head outputs (rng 21), drawn once per frame size / class count and never modified."""
    if ("raw", hw, c) not in _cache:
        _cache[("raw", hw, c)] = post_reference.random_raw(np.random.default_rng(21), BATCH, N, _anchors(hw).shape[0], c=c)
    return _cache[("raw", hw, c)]


def _oracle(cls, box, cov, hw, seed, first, **kw):
    """Per image (oracle debug output, uniforms) of raw head outputs [B,n,A,.]."""
    from oracle import bayes_od, network, philox
    anchors = _anchors(hw)
    out = []
    for img in range(cls.shape[0]):
        u = philox.categorical_uniforms(seed, first + img, anchors.shape[0])
        pred = {"anchors_class_predictions": cls[img], "anchors_box_predictions": box[img],
                "anchors_box_covar_predictions": network.fill_triangular_4(cov[img])}
        out.append((bayes_od.bayes_od_posterior(pred, anchors, u, BAYES_CFG, use_full_covar=True, dtype=np.float64, return_debug=True, **kw), u))
    return out


def _reference(kitti):
    key = ("ref", kitti)
    if key not in _cache:
        hw, c = (KITTI_HW, 4) if kitti else (HW, 8)
        kw = dict(dataset_name="kitti", orig_size=KITTI_ORIG + (3,), net_size=hw + (3,)) if kitti else {}
        _cache[key] = _oracle(*_raw(hw, c), hw, SEED, FIRST, **kw)
    return _cache[key]


def _check_rows(eng, refs, cls, name, min_rows=20, min_kept=100):
    """Posterior class parts of every image against float64 on the rows both sides keep, off a CDF edge.  Returns the maximum."""
    worst = 0.0
    for img, (ref, u) in enumerate(refs):
        got = eng.get_posterior(img)
        rows = eng.get_posterior_class_parts(img)
        assert rows.shape == (len(got["means"]), 3) and rows.dtype == np.float32
        assert ref["keep"].sum() > min_kept and len(rows) > min_kept
        want, _ = clr.posterior_rows_from_debug(ref, cls[img])
        gi, ri = _rows_to_compare(got, ref, u)
        assert len(gi) >= min_rows
        err = np.abs(rows[gi].astype(np.float64) - want[ri])
        worst = max(worst, float(err.max()))
        print("%s image %d: %d rows compared, max |got - float64|: total %.2e aleatoric %.2e epistemic %.2e (bound %.0e); ranges total "
              "%.3g..%.3g epistemic %.3g..%.3g" % (name, img, len(gi), err[:, 0].max(), err[:, 1].max(), err[:, 2].max(), BOUND,
                                                   want[ri, 0].min(), want[ri, 0].max(), want[ri, 2].min(), want[ri, 2].max()))
        assert err.max() <= BOUND
        assert np.all(rows[:, 2] >= 0.0) and np.all(np.isfinite(rows))
    return worst


# ------------------------------------------------------------------------------------------------ 1. posterior rows
@pytest.mark.parametrize("kitti", [False, True], ids=["bdd_c8", "kitti_c4"])
def test_posterior_class_parts_match_float64(kitti):
    """1. bod_set_raw + bod_posterior, bod_get_posterior_class_parts against the restatement, C = 8 and C = 4."""
    hw, c = (KITTI_HW, 4) if kitti else (HW, 8)
    kw = dict(dataset_name="kitti", orig_size=KITTI_ORIG, num_classes=4) if kitti else {}
    eng = _engine(hw=hw, **kw)
    cls, box, cov = _raw(hw, c)
    eng.set_raw(cls, box, cov)
    eng.posterior(seed=SEED, first_image_id=FIRST)
    _check_rows(eng, _reference(kitti), cls, "kitti_c4" if kitti else "bdd_c8")
    eng.close()


# ------------------------------------------------------------------------------------------------ 2. fused epilogue == raw route
_AGG_SCRIPT = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from conftest import ANCHOR_CFG, BAYES_CFG, NMS_CFG
from bayes_od_rc_amd import synthetic
from bayes_od_rc_amd.anchor_generator import FpnAnchorGenerator
from bayes_od_rc_amd.engine import Engine, make_config
h, w, batch, n = (int(v) for v in sys.argv[3:7])
precision, with_stat = sys.argv[7], int(sys.argv[8])
kw = dict(bayes_od_config=BAYES_CFG, nms_config=NMS_CFG, use_full_covar=True, precision=precision, class_parts=True)
weights = synthetic.make_weights(cls_fg_bias=-1.0)
anchors = FpnAnchorGenerator(ANCHOR_CFG).generate_all((h, w, 3))
frames = synthetic.make_frames(batch, h, w, seed=31)
eng = Engine(make_config((h, w), batch=batch, mc_samples=n, **kw))
eng.load_weights(weights)
eng.set_anchors(anchors)
eng.infer(frames, seed=77, first_image_id=5)
out = {"agg_plan": np.int32(eng.aggregating)}
for b in range(batch):
    out["idx%d" % b] = eng.get_posterior(b)["anchor_index"]
    out["rows%d" % b] = eng.get_posterior_class_parts(b)
    out["det%d" % b] = eng.get_detection_class_parts(b)
eng.close()
if with_stat:                                  # a statistics handle: the epilogue's record against stat_from_raw_kernel's
    st = Engine(make_config((h, w), batch=batch, mc_samples=n, mc_statistics=True, **kw))
    st.load_weights(weights)
    st.set_anchors(anchors)
    st.stat_forward(frames, seed=77, first_image_id=5, sample_base=0)
    out["stat_agg_plan"] = np.int32(st.aggregating)
    out["stat_ent"] = st.get_entropy()
    out["stat_cls"] = st.get_statistics()[0]
    st.close()
np.savez(sys.argv[2], **out)
"""


@pytest.mark.parametrize("h,w,batch,n,precision", [(128, 160, 2, 5, "bf16"), (128, 160, 2, 5, "bf16x3"), (128, 160, 2, 5, "f16mx"),
                                                   (96, 160, 1, 30, "bf16")])
def test_fused_epilogue_equals_the_raw_route(tmp_path, h, w, batch, n, precision):
    """2. ent_sum from the classification head's epilogue (AGG_CLS_ENT) against the raw route's loop (BOD_FUSE_AGGREGATION=0), each
    in a process of its own: the same kept set and bit-identical posterior class parts; on the first case also a statistics
    handle's record, the epilogue's against stat_from_raw_kernel's."""
    with_stat = (h, w, batch, n, precision) == (128, 160, 2, 5, "bf16")
    outs = []
    for fuse in ("1", "0"):
        path = str(tmp_path / ("agg%s.npz" % fuse))
        env = dict(os.environ, BOD_FORCE_CONV_TILE="256", BOD_FUSE_AGGREGATION=fuse)
        r = subprocess.run([sys.executable, "-c", _AGG_SCRIPT, ROOT, path, str(h), str(w), str(batch), str(n), precision, str(int(with_stat))],
                           env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
        z = np.load(path)
        outs.append({k: z[k] for k in z.files})
    fused, plain = outs
    assert int(fused["agg_plan"]) == 1 and int(plain["agg_plan"]) == 0
    for b in range(batch):
        assert len(fused["idx%d" % b]) > 30
        assert np.array_equal(fused["idx%d" % b], plain["idx%d" % b])
        assert fused["rows%d" % b].shape == (len(fused["idx%d" % b]), 3)
        assert np.array_equal(fused["rows%d" % b].view(np.uint32), plain["rows%d" % b].view(np.uint32))
        assert np.all(fused["rows%d" % b][:, 0] > 0)
        # (the detections' clusters follow the box means, which the two routes form differently -- Welford against two-pass)
        assert fused["det%d" % b].shape == plain["det%d" % b].shape and len(fused["det%d" % b]) > 0
    if with_stat:
        assert int(fused["stat_agg_plan"]) == 1 and int(plain["stat_agg_plan"]) == 0
        assert np.array_equal(fused["stat_cls"].view(np.uint32), plain["stat_cls"].view(np.uint32))
        assert np.array_equal(fused["stat_ent"].view(np.uint32), plain["stat_ent"].view(np.uint32)) and fused["stat_ent"].min() > 0


# ------------------------------------------------------------------------------------------------ 3. detections
def _members(eng, img, affinity=None, thr=0.5, margin=1e-4):
    """The reference's clusters of the DEVICE's own posterior rows: for every centre of the image the member mask by
    oracle.clustering's rule on the float64 IoU of the device's means (or the caller's affinity columns), and whether no row sits
    within ``margin`` of the threshold (a member there may legitimately differ between fp32 and float64)."""
    means = eng.get_posterior(img)["means"]
    centres = eng.get_nms(img)
    if affinity is None:
        half = means[:, 2:] / np.float32(2.0)                       # the corners as the kernels form them, in float32
        affinity = post_reference.iou_plus1(np.concatenate([means[:, :2] - half, means[:, :2] + half], axis=1))[:, centres].T
    masks = [np.asarray(col) > thr for col in affinity]
    clear = [bool(np.abs(np.asarray(col, np.float64) - thr).min() > margin) for col in affinity]
    return centres, masks, clear


def _check_detections(eng, img, mean_probs, rows, name, affinity=None):
    centres, masks, clear = _members(eng, img, affinity)
    got = eng.get_detection_class_parts(img)
    assert got.shape == (len(centres), 4) and got.dtype == np.float32 and len(centres) > 0
    want = np.array([clr.cluster_rows(mean_probs, rows, m) for m in masks])
    use = np.array(clear)
    assert use.sum() >= 0.9 * len(use)
    err = np.abs(got.astype(np.float64) - want)[use]
    print("%s image %d: %d of %d detections compared (members %d..%d), max |got - float64| %.2e (bound %.0e), spatial part up to %.3g"
          % (name, img, use.sum(), len(use), min(m.sum() for m in masks), max(m.sum() for m in masks), err.max(), BOUND, want[:, 3].max()))
    assert err.max() <= BOUND
    assert np.abs(got[:, 1:].astype(np.float64).sum(axis=1) - got[:, 0]).max() <= 1e-6
    assert got.min() >= 0.0
    return float(err.max())


def _float64_rows_for_device_rows(eng, img, cls_img):
    """Float64 rows and mean_probs of the anchors the device kept (its own kept set, so the clusters match row for row)."""
    idx = eng.get_posterior(img)["anchor_index"]
    cls_sum, ent_sum = clr.statistics(cls_img[:, idx], sample_axis=0)
    return clr.posterior_rows(cls_sum, ent_sum, cls_img.shape[0])


def test_detection_class_parts_match_float64():
    """3. bod_nms + bod_cluster_fuse on the posterior of the random head outputs: every detection against the float64 parts of the
    reference's clusters of the device's own rows; the three parts sum to the total; one image without detections."""
    eng = _engine()
    cls, box, cov = (x.copy() for x in _raw(HW))
    empty = post_reference.random_raw(np.random.default_rng(21), BATCH, N, eng.A, bg=30.0)
    for x, e in zip((cls, box, cov), empty):
        x[1] = e[1]                                            # image 1 keeps nothing
    eng.set_raw(cls, box, cov)
    eng.posterior(seed=SEED, first_image_id=FIRST)
    eng.nms()
    eng.cluster_fuse()
    assert eng.num_kept()[0] > 100 and eng.num_kept()[1] == 0
    rows, pbar = _float64_rows_for_device_rows(eng, 0, cls[0])
    _check_detections(eng, 0, pbar, rows, "detections")
    assert eng.get_detection_class_parts(1).shape == (0, 4) and eng.get_posterior_class_parts(1).shape == (0, 3)
    batch = eng.get_detection_class_parts_batch()
    k0 = len(eng.get_nms(0))
    assert batch.shape == (BATCH, eng.K, 4) and np.array_equal(batch[0, :k0], eng.get_detection_class_parts(0))
    assert not batch[0, k0:].any() and not batch[1].any()
    eng.close()


def test_detection_class_parts_on_the_callers_affinity():
    """3. ... with bod_set_affinity: the members are the caller's one-shot columns, not the IoU's."""
    eng = _engine()
    cls, box, cov = _raw(HW)
    eng.set_raw(cls, box, cov)
    eng.posterior(seed=SEED, first_image_id=FIRST)
    eng.nms()
    m, centres = int(eng.num_kept()[0]), eng.get_nms(0)
    rng = np.random.default_rng(5)
    member = rng.random((len(centres), m)) < 0.2
    member[np.arange(len(centres)), centres] = True
    columns = np.where(member, 0.9, 0.1).astype(np.float32)
    eng.set_affinity(0, columns)
    eng.cluster_fuse()
    rows, pbar = _float64_rows_for_device_rows(eng, 0, cls[0])
    _check_detections(eng, 0, pbar, rows, "affinity", affinity=columns)
    # the injection hooks round-trip and feed the cluster kernel: a cluster of the centre alone returns the centre's row
    eng.set_posterior_class_parts(0, pbar, rows)
    assert np.array_equal(eng.get_posterior_class_parts(0), rows.astype(np.float32))
    alone = np.full((len(centres), m), 0.1, np.float32)
    alone[np.arange(len(centres)), centres] = 0.9
    eng.set_affinity(0, alone)
    eng.cluster_fuse()
    got = eng.get_detection_class_parts(0)
    want = rows[centres].astype(np.float32)
    assert np.abs(got[:, :3] - want).max() <= 1e-6 and np.abs(got[:, 3]).max() <= 1e-6
    eng.close()


# ------------------------------------------------------------------------------------------------ 4. statistics handles
def _stat_engine(hw=HW, n=N, total=2 * N, weights=True, bits=2):
    return _engine(hw=hw, n=n, weights=weights, bits=bits, mc_statistics=True, mc_ensemble_size=total)


def _frames(seed=31):
    from bayes_od_rc_amd import synthetic
    return synthetic.make_frames(BATCH, HW[0], HW[1], seed=seed)


def test_two_passes_merge_to_the_record_of_all_ten_samples():
    """4. Two bod_stat_forward passes of n = 5 (absolute samples 0..4, 5..9): the accumulator's ent_sum, and the posterior class
    parts of the merged record, against float64 on the ten samples' raw logits; get / set round-trip bit for bit."""
    eng = _stat_engine()
    frames = _frames()
    raws = []
    for p in range(2):
        eng.stat_forward(frames, seed=77, first_image_id=5, sample_base=p * N)
        raws.append([x.copy() for x in eng.get_raw()])
    assert eng.stat_samples == 2 * N
    cls, box, cov = (np.concatenate([r[i] for r in raws], axis=1) for i in range(3))
    ent = eng.get_entropy()
    _, want = clr.statistics(cls)
    err = np.abs(ent.astype(np.float64) - want).max() / (2 * N)
    print("ent_sum / K of two merged passes against float64: %.2e (bound %.0e)" % (err, BOUND))
    assert ent.shape == (BATCH, eng.A) and err <= BOUND
    eng.stat_posterior(seed=77, first_image_id=5)
    _check_rows(eng, _oracle(cls, box, cov, HW, 77, 5), cls, "two passes", min_kept=30)
    # round trip: the same bits back, and the posterior after it is the same
    before = [eng.get_posterior_class_parts(b) for b in range(BATCH)]
    rec = eng.get_statistics()
    other = _stat_engine(weights=False)
    other.set_statistics(*rec[:3], samples=rec[3])
    with pytest.raises(ValueError, match="ent_sum"):
        other.stat_posterior(seed=77, first_image_id=5)        # the fourth array has not followed
    other.set_entropy(ent)
    assert np.array_equal(other.get_entropy().view(np.uint32), ent.view(np.uint32))
    other.stat_posterior(seed=77, first_image_id=5)
    for b in range(BATCH):
        assert np.array_equal(other.get_posterior_class_parts(b).view(np.uint32), before[b].view(np.uint32))
    # bod_stat_merge_from and the device-pointer merge carry the fourth array: acc + src
    third = _stat_engine(weights=False)
    third.stat_merge_from(eng)
    third.stat_merge(list(other.stat_device_pointers()) + [other.stat_device_entropy_pointer()], 2 * N)
    assert third.stat_samples == 4 * N and np.array_equal(third.get_entropy(), ent + ent)
    # a source without the option cannot feed a destination with it; the other direction is the three-array merge as ever
    plain = _stat_engine(weights=False, bits=0)
    plain.set_statistics(*rec[:3], samples=rec[3])
    with pytest.raises(ValueError, match="ent_sum"):
        third.stat_merge_from(plain)
    assert third.stat_samples == 4 * N
    plain.stat_merge_from(eng)
    assert plain.stat_samples == 4 * N
    for e in (eng, other, third, plain):
        e.close()


def test_hflip_view_gathers_the_partner_anchors_entropy():
    """4. An identity pass and a mirrored pass in one accumulator: ent_sum equals identity + mirror(flipped pass) bit for bit, and
    the detections' class parts match float64 on the pooled samples."""
    from bayes_od_rc_amd import distributed as bd
    eng = _stat_engine()
    frames = _frames()
    flipped = np.ascontiguousarray(frames[:, :, ::-1])
    perm = bd.mirror_anchor_index(eng.levels, 9)
    eng.stat_forward(frames, seed=77, first_image_id=5, sample_base=0)
    ent_id, raw_id = eng.get_entropy(), [x.copy() for x in eng.get_raw()]
    eng.stat_reset()
    eng.stat_forward(flipped, seed=77, first_image_id=5, sample_base=N)          # the mirrored pass's record in ITS frame
    ent_fl, raw_fl = eng.get_entropy(), [x.copy() for x in eng.get_raw()]
    eng.stat_reset()
    eng.stat_forward(frames, seed=77, first_image_id=5, sample_base=0)
    eng.stat_forward(frames, seed=77, first_image_id=5, sample_base=N, view="hflip")
    got = eng.get_entropy()
    assert not np.array_equal(ent_fl[:, perm], ent_fl)
    assert np.array_equal(got.view(np.uint32), (ent_id + ent_fl[:, perm]).view(np.uint32))
    eng.stat_posterior(seed=77, first_image_id=5)
    eng.nms()
    eng.cluster_fuse()
    pooled = np.concatenate([raw_id[0], raw_fl[0][:, :, perm]], axis=1)          # [B, 2N, A, C] in the frame of the frames as given
    for img in range(BATCH):
        assert eng.num_kept()[img] > 30
        rows, pbar = _float64_rows_for_device_rows(eng, img, pooled[img])
        got_rows = eng.get_posterior_class_parts(img)
        err = np.abs(got_rows.astype(np.float64) - rows).max()
        print("hflip image %d: %d rows, max |got - float64| %.2e (bound %.0e)" % (img, len(rows), err, BOUND))
        assert err <= BOUND
        _check_detections(eng, img, pbar, rows, "hflip")
    eng.close()


# ------------------------------------------------------------------------------------------------ 5. nothing else moves
PARENT_DEVICE_BYTES = 110814666   # Engine.device_bytes of a value-0 handle of the commit before the option, measured at test_nothing_else_moves' geometry


def _infer_everything(eng, frames, seed=77, first=5):
    eng.infer(frames, seed=seed, first_image_id=first)
    out = {"num_kept": eng.num_kept(), "det": eng.get_detections_batch(), "raw": eng.get_raw()}
    for b in range(eng.B):
        out["post%d" % b] = eng.get_posterior(b)
        out["nms%d" % b] = eng.get_nms(b)
    return out


def _assert_same_bits(a, b):
    assert np.array_equal(a["num_kept"], b["num_kept"]) and a["num_kept"].min() > 20
    for x, y in zip(a["raw"], b["raw"]):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    for key in a:
        if key.startswith("post"):
            for k in ("anchor_index", "counts", "score", "means", "covs", "ranking"):
                assert np.array_equal(a[key][k].view(np.uint32), b[key][k].view(np.uint32)), (key, k)
        elif key.startswith("nms"):
            assert np.array_equal(a[key], b[key]) and len(a[key]) > 0
    assert np.array_equal(a["det"]["num"], b["det"]["num"])
    for img, n in enumerate(a["det"]["num"]):
        for k in ("scores", "means", "covs", "counts"):
            assert np.array_equal(a["det"][k][img, :n].view(np.uint32), b["det"][k][img, :n].view(np.uint32)), (img, k)


def test_nothing_else_moves():
    """5. bod_infer with synthetic weights on handles with value 0, 1, 2 and 3: detections, posterior and raw tensors are equal
    bit for bit, the plans are equal (the option adds launches behind the plan's ops, none inside it), value 3 returns value 1's
    covariance parts bit for bit, a value-0 handle holds the device bytes it held before the option existed, and the new getters
    on a handle without the bit fail with a status and a message."""
    frames = _frames()
    engs = {bits: _engine(weights=True, bits=bits) for bits in (0, 1, 2, 3)}
    outs = {bits: _infer_everything(e, frames) for bits, e in engs.items()}
    for bits in (1, 2, 3):
        _assert_same_bits(outs[0], outs[bits])
        assert engs[bits].plan_info() == engs[0].plan_info()
    for b in range(BATCH):
        assert np.array_equal(engs[3].get_posterior_parts(b).view(np.uint32), engs[1].get_posterior_parts(b).view(np.uint32))
        assert np.array_equal(engs[3].get_detection_parts(b).view(np.uint32), engs[1].get_detection_parts(b).view(np.uint32))
        assert np.array_equal(engs[3].get_posterior_class_parts(b).view(np.uint32), engs[2].get_posterior_class_parts(b).view(np.uint32))
        assert np.array_equal(engs[3].get_detection_class_parts(b).view(np.uint32), engs[2].get_detection_class_parts(b).view(np.uint32))
    ba, bk = BATCH * engs[0].A, BATCH * engs[0].K
    print("device bytes: value 0 %d, 1 %d, 2 %d, 3 %d" % tuple(engs[b].device_bytes for b in (0, 1, 2, 3)))
    # the value-0 handle of the commit before the option: measured there at this geometry (128 x 128, batch 2, N = 5, bf16)
    assert engs[0].device_bytes == PARENT_DEVICE_BYTES
    assert engs[2].device_bytes - engs[0].device_bytes >= 4 * ((3 + 8) * ba + 2 * 4 * bk)
    assert engs[3].device_bytes - engs[1].device_bytes == engs[2].device_bytes - engs[0].device_bytes
    for bits in (0, 1):
        e = engs[bits]
        calls = (lambda: e.get_posterior_class_parts(0), lambda: e.set_posterior_class_parts(0, np.zeros((1, 8)), np.zeros((1, 3))),
                 lambda: e.get_detection_class_parts(0), e.get_detection_class_parts_batch, e.device_detection_class_parts_pointer,
                 lambda: e._chk(e.lib.bod_collect_class_parts(e.h, 0, None)), e.get_entropy, e.stat_device_entropy_pointer,
                 lambda: e.set_entropy(np.zeros((BATCH, e.A))), lambda: e.stat_merge_entropy(16, 0))
        for call in calls:
            with pytest.raises(ValueError, match="BOD_PARTS_CLASS"):
                call()
        assert e.lib.bod_record_width(e.h) == 21 + 2 * 8 + 48 * bits
    assert engs[2].lib.bod_record_width(engs[2].h) == 21 + 2 * 8 + 4 and engs[3].lib.bod_record_width(engs[3].h) == 21 + 2 * 8 + 48 + 4
    for call in (lambda: engs[2].get_posterior_parts(0), lambda: engs[2].get_detection_parts(0)):      # class-only: no covariance-parts work
        with pytest.raises(ValueError, match="covariance_parts"):
            call()
    for e in engs.values():
        e.close()


def test_async_tickets_and_records_carry_the_class_parts():
    """5. / records: bod_infer_async tickets collected with bod_collect_class_parts and the world-1 gather's wide rows (values 2 and
    3) equal the synchronous results bit for bit."""
    from bayes_od_rc_amd import distributed as bd
    frames = _frames(17)
    for bits in (2, 3):
        eng = _engine(weights=True, bits=bits)
        eng.infer(frames, seed=5, first_image_id=0)
        want, rows = eng.get_detections_batch(), eng.get_detection_class_parts_batch()
        parts = eng.get_detection_parts_batch() if bits & 1 else None
        width = 21 + 2 * eng.Ccls + (48 if bits & 1 else 0) + 4
        assert eng.lib.bod_record_width(eng.h) == width == bd.record_width(eng.Ccls, cov_parts=bool(bits & 1), class_parts=True)
        got = eng.gather_detections(slot=-1)
        assert got.shape == (1, BATCH, eng.K, width) and want["num"].sum() > 0
        for img, row in enumerate(bd.unpack_records(got[0], eng.Ccls)):
            n = int(want["num"][img])
            assert len(row) == (6 if bits & 1 else 5) and row[-1].shape == (n, 4)
            assert np.array_equal(row[-1], rows[img, :n]) and np.array_equal(row[2], want["covs"][img, :n])
            assert np.array_equal(row[0], want["scores"][img, :n]) and np.array_equal(row[3], want["counts"][img, :n])
            if bits & 1:
                assert np.array_equal(row[4], parts[img, :n])
            assert not got[0, img, n:].any()
        slot = eng.infer_async(frames, seed=5, first_image_id=0)
        assert np.array_equal(eng.gather_detections(slot=slot), got)
        col = eng.collect(slot)
        assert np.array_equal(col["class_parts"].view(np.uint32), rows.view(np.uint32))
        if bits & 1:
            assert np.array_equal(col["cov_parts"][0, :int(want["num"][0])], parts[0, :int(want["num"][0])])
        ptr, shape = eng.device_detection_class_parts_pointer(slot)
        assert ptr != 0 and shape == (BATCH, eng.K, 4)
        eng.close()


def test_pipelines_pass_the_class_parts_through():
    """bayes_od_inference, BayesOdPipeline and EnsemblePipeline (two passes, with and without the hflip view) made with
    class_parts=True return the parts behind their usual values; the last three sum to the first."""
    from bayes_od_rc_amd import constants, inference_utils, synthetic
    from bayes_od_rc_amd.model import RetinaNetModel
    model = RetinaNetModel({"output_names": ["classification", "regression", "regression_covar"], "mc_dropout_samples": N,
                            "header": {"dropout_rate": 0.3, "num_classes": 7, "anchors_per_location": 9}})
    model.load_weights(synthetic.make_weights(cls_fg_bias=-1.0))
    frames, anchors = _frames(), _anchors(HW)
    sample = {constants.IMAGE_NORMALIZED_KEY: frames[:1], constants.ANCHORS_KEY: anchors}
    out = inference_utils.bayes_od_inference(model, sample, BAYES_CFG, NMS_CFG, use_full_covar=True, seed=77, image_id=5,
                                             return_iou=False, class_parts=True)
    assert len(out) == 6 and out[5].shape == (len(out[2]), 3 + 8) and len(out[2]) > 20
    assert np.abs(out[5][:, 1] + out[5][:, 2] - out[5][:, 0]).max() <= 1e-6 and np.abs(out[5][:, 3:].sum(axis=1) - 1.0).max() <= 1e-5
    pipes = [inference_utils.BayesOdPipeline(model, HW, BATCH, BAYES_CFG, NMS_CFG, anchors=anchors, class_parts=True),
             inference_utils.EnsemblePipeline([model], HW, BATCH, BAYES_CFG, NMS_CFG, N, passes=2, anchors=anchors, class_parts=True),
             inference_utils.EnsemblePipeline([model, model], HW, BATCH, BAYES_CFG, NMS_CFG, N, anchors=anchors, views=("identity", "hflip"),
                                              covariance_parts=True, class_parts=True)]
    for pipe, width in zip(pipes, (5, 5, 6)):
        dets = pipe(frames, seed=77, first_image_id=5)
        assert len(dets) == BATCH
        for det in dets:
            assert len(det) == width and len(det[2]) > 0 and det[-1].shape == (len(det[2]), 4)
            assert np.abs(det[-1][:, 1:].sum(axis=1) - det[-1][:, 0]).max() <= 1e-6 and det[-1].min() >= 0 and det[-1][:, 0].max() <= np.log(8.0) + 1e-6
            if width == 6:
                assert det[4].shape == (len(det[2]), 3, 4, 4)


def test_two_call_route_returns_the_detections_class_parts():
    """bayes_od_inference(class_parts=True) then bayes_od_clustering(class_parts=its sixth value), the reference's two calls: the
    [K,4] array comes last and meets float64 on the reference's clusters of the rows that went in -- on the handle of the first
    call, on a post-processing handle of the call's own, and with a caller's affinity matrix; without the argument four values."""
    from bayes_od_rc_amd import constants, inference_utils, synthetic
    from bayes_od_rc_amd.model import RetinaNetModel
    model = RetinaNetModel({"output_names": ["classification", "regression", "regression_covar"], "mc_dropout_samples": N,
                            "header": {"dropout_rate": 0.3, "num_classes": 7, "anchors_per_location": 9}})
    model.load_weights(synthetic.make_weights(cls_fg_bias=-1.0))
    sample = {constants.IMAGE_NORMALIZED_KEY: _frames()[:1], constants.ANCHORS_KEY: _anchors(HW)}
    counts, means, covs, centres, iou, cparts, eng = inference_utils.bayes_od_inference(
        model, sample, BAYES_CFG, NMS_CFG, use_full_covar=True, seed=77, image_id=5, class_parts=True, return_engine=True)
    m = len(counts)
    assert cparts.shape == (m, 11) and m > 30 and len(centres) > 3 and iou.shape == (m, m)
    rows, pbar = cparts[:, :3].astype(np.float64), cparts[:, 3:].astype(np.float64)
    rng = np.random.default_rng(9)
    custom = np.where(rng.random((m, m)) < 0.2, 0.9, 0.1)
    custom[centres, centres] = 0.9
    for name, aff, thr, engine in (("own handle", iou, 0.5, eng), ("standalone", iou, 0.5, None), ("affinity", custom, 0.7, None)):
        out = inference_utils.bayes_od_clustering(counts, means, covs, centres, aff, thr, engine=engine, class_parts=cparts)
        assert len(out) == 5 and out[4].shape == (len(centres), 4) and out[4].dtype == np.float32
        clear = np.abs(np.asarray(aff, np.float64)[:, centres] - thr).min(axis=0) > 1e-4
        want = clr.cluster_class_parts(pbar, rows, centres, aff, thr)
        err = np.abs(out[4].astype(np.float64) - want)[clear]
        print("two-call route (%s): %d of %d detections compared, max |got - float64| %.2e (bound %.0e)" % (name, clear.sum(), len(clear), err.max(), BOUND))
        assert clear.sum() >= 0.9 * len(clear) and err.max() <= BOUND
        assert np.abs(out[4][:, 1:].sum(axis=1) - out[4][:, 0]).max() <= 1e-6
        plain = inference_utils.bayes_od_clustering(counts, means, covs, centres, aff, thr, engine=engine)
        assert len(plain) == 4 and all(np.array_equal(a, b) for a, b in zip(plain, out[:4]))
    on_the_fly = inference_utils.bayes_od_clustering(counts, means, covs, centres, None, 0.5, engine=eng, class_parts=cparts)
    assert on_the_fly[4].shape == (len(centres), 4)
    with pytest.raises(ValueError, match="class_parts"):
        inference_utils.bayes_od_clustering(counts, means, covs, centres, iou, 0.5, class_parts=cparts[:-1])
    with pytest.raises(ValueError, match="class_parts"):
        inference_utils.bayes_od_clustering(counts, means, covs, centres, iou, 0.5, engine=_engine(bits=0), class_parts=cparts)
    empty = inference_utils.bayes_od_clustering(counts, means, covs, np.zeros(0, np.int32), iou, 0.5, class_parts=cparts)
    assert len(empty) == 5 and empty[4].shape == (0, 4)


# ------------------------------------------------------------------------------------------------ 6. gather
def test_two_ranks_on_one_gpu_gather_wide_rows(tmp_path):
    """6. StatShardedEngine with class_parts over two processes (both on this GPU, gloo; tests/tools/class_parts_shard_worker.py):
    the records carry ent_sum through the all-gather, the detections' class parts are equal across the ranks bit for bit, and the
    wide rows every rank packs arrive on rank 0 through gather_records as they were sent."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    worker = os.path.join(ROOT, "tests", "tools", "class_parts_shard_worker.py")
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
    assert "CLASS_PARTS_SHARD_OK" in outs[0][0], outs[0]
    a, b = np.load(str(tmp_path / "rank0.npz")), np.load(str(tmp_path / "rank1.npz"))
    assert sorted(a.files) == sorted(b.files) and len(a.files) >= 4
    for k in a.files:
        assert np.array_equal(a[k], b[k]), k
    assert a["det0_class_parts"].shape[0] > 0 and a["det0_class_parts"].shape[1] == 4
