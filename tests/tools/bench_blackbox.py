#!/usr/bin/env python3
"""Measurements of DESIGN.md 9.18 (python tests/tools/bench_blackbox.py [cls foreground bias] [batch]): the full step under
bod_set_uncertainty_method's two methods, interleaved on one handle pair (one handle per method, same weights and frames), and the
two black-box stages alone on the head outputs of that step, at 512x512, N = 10, batch 64: 5 x 20 calls by the host clock.  The
card's clock and power at the start of the run are noted, and the HBM the method adds to a handle."""
import os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from conftest import ANCHOR_CFG, BAYES_CFG, NMS_CFG
from bayes_od_rc_amd import synthetic
from bayes_od_rc_amd.anchor_generator import FpnAnchorGenerator
from bayes_od_rc_amd.engine import Engine, make_config

FG = float(sys.argv[1]) if len(sys.argv) > 1 else -3.2
B = int(sys.argv[2]) if len(sys.argv) > 2 else 64
hw, n = (512, 512), 10


def card_state():
    """One line of the card's clocks and power (read only), or why it could not be read."""
    why = "no output"
    for cmd in (["rocm-smi", "--showclocks", "--showpower"], ["amd-smi", "metric", "--clock", "--power"]):
        try:
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=30).stdout
        except (OSError, subprocess.SubprocessError) as e:
            why = str(e)
            continue
        lines = [l.strip() for l in out.splitlines() if any(k in l.lower() for k in ("sclk", "gfx", "power", "mclk"))]
        if lines:
            return " | ".join(lines[:8])
    return "not readable here (%s)" % why


def clock(f, eng, it):
    """ms per call: host clock over `it` back-to-back calls ending in one synchronise"""
    t0 = time.perf_counter()
    for _ in range(it):
        f()
    eng.synchronize()
    return (time.perf_counter() - t0) / it * 1e3


def line(name, v):
    print("B=%d %-28s %s ms (median %.3f)" % (B, name, " ".join("%.3f" % x for x in v), float(np.median(v))), flush=True)


print("card at start: " + card_state(), flush=True)
anchors = FpnAnchorGenerator(ANCHOR_CFG).generate_all((hw[0], hw[1], 3))
w = synthetic.make_weights(cls_fg_bias=FG)
frames = synthetic.make_frames(min(B, 64), hw[0], hw[1], seed=1)
frames = np.concatenate([frames] * (B // len(frames)))[:B]
engines = {}
for method in ("bayes_od", "black_box"):
    eng = Engine(make_config(hw, batch=B, mc_samples=n, bayes_od_config=BAYES_CFG, nms_config=NMS_CFG, use_full_covar=True))
    eng.load_weights(w)
    eng.set_anchors(anchors)
    eng.upload_images(frames)
    engines[method] = eng
before = engines["black_box"].device_bytes
engines["black_box"].set_uncertainty_method("black_box")
steps = {m: (lambda e=e: e.infer(None, seed=3, first_image_id=0)) for m, e in engines.items()}
for m in steps:
    for _ in range(3):
        steps[m]()
    engines[m].synchronize()
after = engines["black_box"].device_bytes                   # (the first black-box step also allocates the per-sample head outputs)
out = {m: [] for m in steps}
for rep in range(5):
    for m in steps:                                         # interleaved: one box state for both
        out[m].append(clock(steps[m], engines[m], 20))
bb = engines["black_box"]
s1 = [clock(bb.blackbox_samples, bb, 20) for _ in range(5)]
s2 = [clock(bb.blackbox_merge, bb, 20) for _ in range(5)]
num_bb = bb.get_detections_batch()["num"]
members = bb.get_detection_merge_terms_batch()["members"]
pool = np.mean([len(bb.get_sample_detections(b, s)["anchor_index"]) for b in range(min(B, 4)) for s in range(n)])
num_bo = engines["bayes_od"].get_detections_batch()["num"]
line("step bayes_od", out["bayes_od"])
line("step black_box", out["black_box"])
line("stage 1 (blackbox_samples)", s1)
line("stage 2 (blackbox_merge)", s2)
print("B=%d detections per image: bayes_od %.1f, black_box %.1f; sample detections per (image, sample) %.1f; members per detection %.2f"
      % (B, num_bo.mean(), num_bb.mean(), pool, members.sum() / max(num_bb.sum(), 1)), flush=True)
print("B=%d HBM held: %.1f MiB before the switch, %.1f MiB after the first black-box steps (+%.1f MiB)"
      % (B, before / 2 ** 20, after / 2 ** 20, (after - before) / 2 ** 20), flush=True)
for e in engines.values():
    e.close()
