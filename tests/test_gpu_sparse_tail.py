"""The sparse tail (engine.hip build_plan, SparseTailArgs in kernels.h): on the aggregating bf16 plan the box-regression head's last
layer and the covariance head's last layer run behind the keep flags, over the pixels with a kept anchor only.  Everything the
posterior reads of those heads belongs to kept anchors, so detections and posteriors must equal the dense plan's
(BOD_SPARSE_TAIL=0) bit for bit: square and non-square frames (pyramid widths that are not multiples of 4), N = 10 and 30, a
frame that keeps nothing, a foreground bias at which nearly every anchor is kept (the row table's worst case), and two-slot pipelining
(whose later calls find the earlier calls' statistics in the buffers: stale entries of anchors not kept must stay unread).
pipeline_overlap handles (experimental) keep the dense plan.  The keep sets here are whatever the random network fires on;
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

def engine(hw, b, n, bias, sparse, **kw):
    os.environ["BOD_SPARSE_TAIL"] = "1" if sparse else "0"         # (read when the plan is built: with the weights)
    try:
        eng = Engine(make_config(hw, batch=b, mc_samples=n, **kw))
        eng.load_weights(synthetic.make_weights(cls_fg_bias=bias))
        eng.set_anchors(FpnAnchorGenerator(ACFG).generate_all((hw[0], hw[1], 3)))
        info = eng.plan_info()
    finally:
        os.environ.pop("BOD_SPARSE_TAIL")
    assert info["aggregating"] and info["sparse_tail"] == sparse, info
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
    for sparse in (True, False):
        eng = engine(hw, b, n, bias, sparse)
        eng.infer(frames, seed=77, first_image_id=3)
        outs.append(outputs(eng))
        eng.close()
    same(tag, outs[0], outs[1])
    print(tag, "kept", outs[0]["kept"].tolist(), flush=True)
    return outs[0]["kept"]

def async_case(tag, hw, b, n, bias):
    frames = synthetic.make_frames(b, hw[0], hw[1], seed=9)
    res = []
    for sparse in (True, False):
        eng = engine(hw, b, n, bias, sparse)
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
    same(tag, res[0], res[1])
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
def test_sparse_tail_is_bit_identical_to_dense(case):
    env = dict(os.environ, BOD_FORCE_CONV_TILE="256")
    r = subprocess.run([sys.executable, "-c", SCRIPT % {"root": ROOT}, case], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "DONE" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
