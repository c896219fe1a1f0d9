#!/usr/bin/env python3
"""Measurements of profiles/cov_parts_ab.txt (python tests/tools/bench_cov_parts.py [cls foreground bias] [batches]): the step of a
handle with bod_config.covariance_parts beside one without, and the two launches the option adds -- post_parts_kernel and
cluster_parts_kernel -- as the difference of the stage that holds them, at B = 64 and 512, 512x512, N = 10."""
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
hw, n = (512, 512), 10
anchors = FpnAnchorGenerator(ANCHOR_CFG).generate_all((hw[0], hw[1], 3))
w = synthetic.make_weights(cls_fg_bias=FG)


def handle(b, parts, frames):
    eng = Engine(make_config(hw, batch=b, mc_samples=n, bayes_od_config=BAYES_CFG, nms_config=NMS_CFG, use_full_covar=True, covariance_parts=parts))
    eng.load_weights(w)
    eng.set_anchors(anchors)
    eng.upload_images(frames)
    return eng


def clock(f, eng, it):
    """ms per call: host clock over `it` back-to-back calls ending in one synchronise"""
    t0 = time.perf_counter()
    for _ in range(it):
        f()
    eng.synchronize()
    return (time.perf_counter() - t0) / it * 1e3


def measure(eng, name, b):
    step = lambda: eng.infer(None, seed=3, first_image_id=0)
    post = lambda: eng.posterior(seed=3, first_image_id=0)
    for _ in range(3):
        step()
    eng.synchronize()
    out = {}
    for rep in range(3):
        out.setdefault("step", []).append(clock(step, eng, 5))
        out.setdefault("posterior", []).append(clock(post, eng, 20))          # (keep + compaction + fusion [+ parts] on the step's statistics)
        eng.nms()
        out.setdefault("cluster", []).append(clock(eng.cluster_fuse, eng, 20))      # (cluster_fuse_kernel [+ cluster_parts_kernel])
    kept = eng.num_kept()
    print("B=%d %-5s step %s ms  posterior stage %s ms  cluster stage %s ms  kept anchors per image %.0f  device GB %.2f"
          % (b, name, " ".join("%.2f" % v for v in out["step"]), " ".join("%.3f" % v for v in out["posterior"]),
             " ".join("%.3f" % v for v in out["cluster"]), kept.mean(), eng.device_bytes / 1e9), flush=True)
    return {k: float(np.median(v)) for k, v in out.items()}, float(kept.mean())


for b in BATCHES:
    frames = synthetic.make_frames(min(b, 64), hw[0], hw[1], seed=1)
    frames = np.concatenate([frames] * (b // len(frames)))[:b]
    res = {}
    for name, parts in (("off", False), ("on", True), ("off", False), ("on", True)) if b <= 64 else (("off", False), ("on", True)):
        eng = handle(b, parts, frames)                   # one handle at a time: two of 512 frames do not fit beside each other
        r, kept = measure(eng, name, b)
        res.setdefault(name, []).append(r)
        eng.close()
    off = {k: np.mean([r[k] for r in res["off"]]) for k in res["off"][0]}
    on = {k: np.mean([r[k] for r in res["on"]]) for k in res["on"][0]}
    # the per-anchor kernel reads a kept slot's statistics rows (box moments 64 B, covariance sums 40 B, anchor 16 B, its index 4 B) and
    # writes 120 B; 8 TB/s HBM3E peak
    floor_ms = b * kept * (64 + 40 + 16 + 4 + 120) / 8e12 * 1e3
    print("B=%d: step off %.2f on %.2f ms (%+.2f %%); post_parts_kernel %.3f ms (byte floor %.5f ms for %.0f kept slots per image); "
          "cluster_parts_kernel %.3f ms" % (b, off["step"], on["step"], 100 * (on["step"] / off["step"] - 1), on["posterior"] - off["posterior"],
                                            floor_ms, kept, on["cluster"] - off["cluster"]), flush=True)
