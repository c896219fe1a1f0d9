#!/usr/bin/env python3
"""Measurements of profiles/stat_merge_ab.txt (python tests/tools/bench_stat_merge.py [cls foreground bias]): stat_merge_kernel at B = 512, 512x512, and a 5-member x n = 2 ensemble beside a
single N = 10 handle on the dense plan (context only)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from conftest import ANCHOR_CFG, BAYES_CFG, NMS_CFG
from bayes_od_rc_amd import synthetic
from bayes_od_rc_amd.anchor_generator import FpnAnchorGenerator
from bayes_od_rc_amd.engine import Engine, make_config
from bayes_od_rc_amd.inference_utils import EnsemblePipeline
from bayes_od_rc_amd.model import RetinaNetModel

FG = float(sys.argv[1]) if len(sys.argv) > 1 else -1.0
hw = (512, 512)
# ---- merge kernel
B = 512
dst = Engine(make_config(hw, batch=B, mc_samples=2, mc_statistics=True))
src = Engine(make_config(hw, batch=B, mc_samples=2, mc_statistics=True))
dst.set_statistics(None, None, None, samples=5)
src.set_statistics(None, None, None, samples=5)
ptrs = src.stat_device_pointers()
for _ in range(3):
    dst.stat_merge(ptrs, 5)
dst.synchronize()
for rep in range(3):
    it = 20
    t0 = time.perf_counter()
    for _ in range(it):
        dst.stat_merge(ptrs, 5)
    dst.synchronize()
    ms = (time.perf_counter() - t0) / it * 1e3
    byts = 408.0 * B * dst.A
    print("stat_merge_kernel B=%d A=%d: %.3f ms per merge (host clock over %d back-to-back launches + synchronise), %.2f GB -> %.2f TB/s"
          % (B, dst.A, ms, it, byts / 1e9, byts / ms / 1e9), flush=True)
dst.close(); src.close()

# ---- ensemble context
B = 64
anchors = FpnAnchorGenerator(ANCHOR_CFG).generate_all((hw[0], hw[1], 3))
frames = synthetic.make_frames(B, hw[0], hw[1], seed=1)
w = synthetic.make_weights(cls_fg_bias=FG)
def model(n):
    m = RetinaNetModel({"output_names": ["classification", "regression", "regression_covar"], "mc_dropout_samples": n,
                        "header": {"dropout_rate": 0.3, "num_classes": 7, "anchors_per_location": 9}})
    m.load_weights(w)
    return m
pipe = EnsemblePipeline([model(2) for _ in range(5)], hw, B, BAYES_CFG, NMS_CFG, 2, anchors=anchors)
print("ensemble member plan:", pipe.engine.plan_info(), flush=True)
os.environ["BOD_SPARSE_TAIL"] = "0"
single = Engine(make_config(hw, batch=B, mc_samples=10, bayes_od_config=BAYES_CFG, nms_config=NMS_CFG, use_full_covar=True))
single.load_weights(w)
del os.environ["BOD_SPARSE_TAIL"]
single.set_anchors(anchors)
print("single handle plan:", single.plan_info(), flush=True)
pipe.engine.upload_images(frames)
single.upload_images(frames)
def run_pipe():
    pipe(None, seed=3, first_image_id=0)
def run_single():
    single.infer(None, seed=3, first_image_id=0)
    single.synchronize()
for f in (run_pipe, run_single, run_pipe, run_single):
    f()
for rep in range(3):
    for name, f in (("ensemble 5 x n=2 (EnsemblePipeline, incl. per-image detection copies)", run_pipe), ("single N=10, dense plan (infer + synchronise)", run_single)):
        it = 5
        t0 = time.perf_counter()
        for _ in range(it):
            f()
        dt = (time.perf_counter() - t0) / it
        print("rep %d  %-75s %.1f ms per batch of %d -> %.1f frames/s" % (rep, name, dt * 1e3, B, B / dt), flush=True)
print("kept anchors per image (single):", single.num_kept()[:4], flush=True)
