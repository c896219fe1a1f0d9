#!/usr/bin/env python3
"""Measurements of DESIGN.md 9.17 (python tests/tools/bench_merge.py [cls foreground bias] [batches]): the cluster stage of ONE
handle on ONE posterior under the three merge methods of bod_set_merge_method -- cluster_fuse_kernel (bayes) and
cluster_merge_kernel (centre, mixture) -- interleaved, and the full step under the default method, at B = 64 and 512, 512x512,
N = 10."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from conftest import ANCHOR_CFG, BAYES_CFG, NMS_CFG
from bayes_od_rc_amd import synthetic
from bayes_od_rc_amd.anchor_generator import FpnAnchorGenerator
from bayes_od_rc_amd.engine import Engine, make_config

FG = float(sys.argv[1]) if len(sys.argv) > 1 else -3.2
BATCHES = [int(v) for v in sys.argv[2].split(",")] if len(sys.argv) > 2 else [64, 512]
METHODS = ("bayes", "centre", "mixture")
hw, n, C = (512, 512), 10, 8
anchors = FpnAnchorGenerator(ANCHOR_CFG).generate_all((hw[0], hw[1], 3))
w = synthetic.make_weights(cls_fg_bias=FG)


def clock(f, eng, it):
    """ms per call: host clock over `it` back-to-back calls ending in one synchronise"""
    t0 = time.perf_counter()
    for _ in range(it):
        f()
    eng.synchronize()
    return (time.perf_counter() - t0) / it * 1e3


for b in BATCHES:
    frames = synthetic.make_frames(min(b, 64), hw[0], hw[1], seed=1)
    frames = np.concatenate([frames] * (b // len(frames)))[:b]
    eng = Engine(make_config(hw, batch=b, mc_samples=n, bayes_od_config=BAYES_CFG, nms_config=NMS_CFG, use_full_covar=True))
    eng.load_weights(w)
    eng.set_anchors(anchors)
    eng.upload_images(frames)
    step = lambda: eng.infer(None, seed=3, first_image_id=0)
    for _ in range(3):
        step()
    eng.synchronize()
    steps = [clock(step, eng, 5) for _ in range(5)]                 # default method: the path every existing caller takes
    eng.posterior(seed=3, first_image_id=0)                         # the step's posterior and centres, left in place for the stage
    eng.nms()
    out = {m: [] for m in METHODS}
    for m in METHODS:                                               # (the first non-default call allocates the term buffers)
        eng.set_merge_method(m)
        eng.cluster_fuse()
    eng.synchronize()
    for rep in range(5):
        for m in METHODS:                                           # interleaved: one box state for all three
            eng.set_merge_method(m)
            out[m].append(clock(eng.cluster_fuse, eng, 20))
    members = eng.get_detection_merge_terms_batch()["members"]
    num = eng.get_detections_batch()["num"]
    eng.set_merge_method("bayes")
    kept = eng.num_kept()
    print("B=%d step (bayes) %s ms; kept anchors per image %.0f, detections per image %.1f, members per detection %.2f"
          % (b, " ".join("%.2f" % v for v in steps), kept.mean(), num.mean(), members.sum() / max(num.sum(), 1)), flush=True)
    for m in METHODS:
        print("B=%d cluster stage %-8s %s ms (median %.3f)" % (b, m, " ".join("%.3f" % v for v in out[m]), float(np.median(out[m]))), flush=True)
    eng.close()
