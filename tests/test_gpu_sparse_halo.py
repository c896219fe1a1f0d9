"""The sparse halo (engine.hip build_plan, sparse_tables.h): on the aggregating bf16 plan box layer 1 and covariance layer 2 run behind
the keep flags, over the 3x3 dilation of the sparse tail's pixels only, and keep dense raw-only launches for raw forwards.  Detections,
posteriors, a posterior under another seed (the raw re-run) and the raw head outputs must equal the tail-only plan's
(BOD_SPARSE_HALO=0) and the dense plan's (BOD_SPARSE_TAIL=0) bit for bit: square and non-square frames, N = 10 and 30, a frame that
keeps nothing, a nearly-all-kept batch and two-slot pipelining.  The keep sets here are whatever the random network fires on;
test_gpu_sparse_masks.py chooses them through a class layer that ignores its input (a bias f keeps each pixel with one probability)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCRIPT = r"""
import os, sys
import numpy as np
sys.path.insert(0, %(root)r)
from bayes_od_rc_amd import synthetic
from bayes_od_rc_amd.anchor_generator import FpnAnchorGenerator
from bayes_od_rc_amd.engine import Engine, make_config

ACFG = {"layers": [3, 4, 5, 6, 7], "aspect_ratios": [[1.0, 1.0], [1.0, 2.0], [2.0, 1.0]], "scales": [1.0, 1.26, 1.59]}

PLANS = ("halo", "tail", "dense")

def engine(hw, b, n, bias, plan, **kw):
    os.environ["BOD_SPARSE_TAIL"] = "0" if plan == "dense" else "1"      # (read when the plan is built: with the weights)
    os.environ["BOD_SPARSE_HALO"] = "1" if plan == "halo" else "0"
    try:
        eng = Engine(make_config(hw, batch=b, mc_samples=n, **kw))
        eng.load_weights(synthetic.make_weights(cls_fg_bias=bias))
        eng.set_anchors(FpnAnchorGenerator(ACFG).generate_all((hw[0], hw[1], 3)))
        info = eng.plan_info()
    finally:
        os.environ.pop("BOD_SPARSE_TAIL")
        os.environ.pop("BOD_SPARSE_HALO")
    assert info["aggregating"] and info["sparse_tail"] == (plan != "dense") and info["sparse_halo"] == (plan == "halo"), info
    return eng

def same(tag, x, y):
    assert type(x) == type(y), tag
    if isinstance(x, dict):
        assert set(x) == set(y), tag
        for k in x:
            same(tag + "." + k, x[k], y[k])
    elif isinstance(x, (tuple, list)):
        assert len(x) == len(y), tag
        for i, (u, v) in enumerate(zip(x, y)):
            same("%%s[%%d]" %% (tag, i), u, v)
    else:
        u, v = np.asarray(x), np.asarray(y)
        assert u.shape == v.shape and u.dtype == v.dtype, (tag, u.shape, v.shape)
        assert np.array_equal(u.view(np.uint8), v.view(np.uint8)), tag

def outputs(eng):
    return {"kept": eng.num_kept(), "post": [eng.get_posterior(i) for i in range(eng.B)],
            "det": [eng.get_detections(i) for i in range(eng.B)]}

def sync_case(tag, hw, b, n, bias, blank=None):
    frames = synthetic.make_frames(b, hw[0], hw[1], seed=5)
    if blank is not None:
        frames[blank] = 0.0
    outs = []
    for plan in PLANS:
        eng = engine(hw, b, n, bias, plan)
        eng.infer(frames, seed=77, first_image_id=3)
        o = outputs(eng)
        # a posterior under another seed and first image: the box / covariance statistics of other anchors, from the raw re-run
        # (box layer 1 and covariance layer 2 densely again, then the last layers' raw flavour)
        eng.posterior(seed=78, first_image_id=5)
        o["post2"] = [eng.get_posterior(i) for i in range(eng.B)]
        o["raw"] = list(eng.get_raw())
        outs.append(o)
        eng.close()
    # (the dense plan serves that posterior from its aggregated statistics, the sparse plans from the raw tensors: compared between
    # the two sparse plans)
    same(tag + ".post2", outs[0].pop("post2"), outs[1].pop("post2"))
    outs[2].pop("post2")
    for o in outs[1:]:
        same(tag, outs[0], o)
    print(tag, "kept", outs[0]["kept"].tolist(), flush=True)
    return outs[0]["kept"]

def async_case(tag, hw, b, n, bias):
    frames = synthetic.make_frames(b, hw[0], hw[1], seed=9)
    res = []
    for plan in PLANS:
        eng = engine(hw, b, n, bias, plan)
        eng.upload_images(frames)
        got, pending = [], []
        for i in range(4):
            pending.append(eng.infer_async(None, seed=i, first_image_id=10 * i))
            if len(pending) > 1:
                got.append(eng.collect(pending.pop(0)))
        got.append(eng.collect(pending.pop(0)))
        eng.synchronize()
        res.append(got)
        eng.close()
    for r in res[1:]:
        same(tag, res[0], r)
    print(tag, "ok", flush=True)

case = sys.argv[1]
if case == "shapes":
    sync_case("square_n10", (128, 128), 32, 10, -3.2, blank=1)
    sync_case("nonsquare_n30", (96, 160), 12, 30, -3.2)
    sync_case("nonsquare_n10", (136, 200), 24, 10, -3.2)
elif case == "extremes":
    k = sync_case("keep_nothing", (128, 128), 32, 10, -40.0)
    assert (k == 0).all(), k
    k = sync_case("keep_almost_all", (96, 160), 24, 10, 8.0)
    assert k.min() > 0.5 * 9 * (12 * 20 + 6 * 10 + 3 * 5 + 2 * 3 + 1 * 2), k
elif case == "pipelined":
    async_case("infer_async", (128, 128), 32, 10, -3.2)

print("DONE", flush=True)
"""



@pytest.mark.parametrize("case", ["shapes", "extremes", "pipelined"])
def test_sparse_halo_is_bit_identical_to_tail_and_dense(case):
    env = dict(os.environ, BOD_FORCE_CONV_TILE="256")
    r = subprocess.run([sys.executable, "-c", SCRIPT % {"root": ROOT}, case], env=env, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0 and "DONE" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
