#!/usr/bin/env python3
"""Measurements of profiles/class_parts_ab.txt (python tests/tools/bench_class_parts.py [cls foreground bias] [batches]): the step
of a handle with BOD_PARTS_CLASS in bod_config.covariance_parts beside one without, and what the option adds -- the tower kernel's
launches (device events around the row-reuse tower launches: the classification head's aggregating launch is one of them, with
one more 4-byte store per anchor), post_class_parts_kernel and cluster_class_parts_kernel as the difference of the stage that
holds them -- at B = 64 and 512, 512x512, N = 10."""
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
hw, n, C = (512, 512), 10, 8
anchors = FpnAnchorGenerator(ANCHOR_CFG).generate_all((hw[0], hw[1], 3))
w = synthetic.make_weights(cls_fg_bias=FG)


def handle(b, on, frames):
    eng = Engine(make_config(hw, batch=b, mc_samples=n, bayes_od_config=BAYES_CFG, nms_config=NMS_CFG, use_full_covar=True, class_parts=on))
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
        eng.profile_begin(which=1)                                  # device events around the tower kernel's launches of 5 steps
        for _ in range(5):
            step()
        out.setdefault("tower", []).append(eng.profile_end()["head_conv_ms"] / 5)
        out.setdefault("posterior", []).append(clock(post, eng, 20))          # (keep + compaction + fusion [+ class parts] on the step's statistics)
        eng.nms()
        out.setdefault("cluster", []).append(clock(eng.cluster_fuse, eng, 20))      # (cluster_fuse_kernel [+ cluster_class_parts_kernel])
    kept = eng.num_kept()
    print("B=%d %-5s step %s ms  tower launches %s ms  posterior stage %s ms  cluster stage %s ms  kept anchors per image %.0f  device GB %.2f"
          % (b, name, " ".join("%.2f" % v for v in out["step"]), " ".join("%.3f" % v for v in out["tower"]),
             " ".join("%.3f" % v for v in out["posterior"]), " ".join("%.3f" % v for v in out["cluster"]), kept.mean(), eng.device_bytes / 1e9), flush=True)
    return {k: float(np.median(v)) for k, v in out.items()}, float(kept.mean())


for b in BATCHES:
    frames = synthetic.make_frames(min(b, 64), hw[0], hw[1], seed=1)
    frames = np.concatenate([frames] * (b // len(frames)))[:b]
    res = {}
    for name, on in (("off", False), ("on", True), ("off", False), ("on", True)) if b <= 64 else (("off", False), ("on", True)):
        eng = handle(b, on, frames)                      # one handle at a time: two of 512 frames do not fit beside each other
        r, kept = measure(eng, name, b)
        res.setdefault(name, []).append(r)
        eng.close()
    off = {k: np.mean([r[k] for r in res["off"]]) for k in res["off"][0]}
    on = {k: np.mean([r[k] for r in res["on"]]) for k in res["on"][0]}
    # byte floors at the 8 TB/s HBM3E peak: the launch writes 4 bytes per anchor on top of cls_sum's 32; the per-slot kernel reads a
    # kept slot's index, cls_sum row and ent_sum and writes C + 3 floats
    launch_floor = b * anchors.shape[0] * 4 / 8e12 * 1e3
    slot_floor = b * kept * (4 + 4 * C + 4 + 4 * (C + 3)) / 8e12 * 1e3
    print("B=%d: step off %.2f on %.2f ms (%+.2f %%); tower launches off %.3f on %.3f ms (added %.3f, byte floor of the added store %.4f ms); "
          "post_class_parts_kernel %.3f ms (byte floor %.5f ms for %.0f kept slots per image); cluster_class_parts_kernel %.3f ms"
          % (b, off["step"], on["step"], 100 * (on["step"] / off["step"] - 1), off["tower"], on["tower"], on["tower"] - off["tower"], launch_floor,
             on["posterior"] - off["posterior"], slot_floor, kept, on["cluster"] - off["cluster"]), flush=True)
