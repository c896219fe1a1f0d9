#!/usr/bin/env python3
"""What producing the anchor targets costs a training step.  Three legs, alternated in one process after both routes are warm:

  A       bod_train_step on pre-built dense targets (host arrays: the step with its target copies, nothing else)
  A-host  sample_builder.create_sample_dict for the minibatch (host only): what a user waited for before each A
  B       bod_train_step_boxes: the targets are assigned on the device from the ground-truth boxes, inside the step

The frames are device-resident for A and B alike; every timed window ends in a device synchronise (the out6 read-back of each
step is one).  Reported: median and round-to-round spread (max - min of the round medians) of each leg, and whether
B <= A + spread(A).  usage: bench_train_targets.py [--rounds 5] [--steps 20] [--cases 512x512x5,720x1280x30] [--batch 3]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np

from bayes_od_rc_amd import constants, synthetic
from bayes_od_rc_amd.engine import Engine, make_config
from bayes_od_rc_amd.sample_builder import create_sample_dict

ACFG = {'layers': [3, 4, 5, 6, 7], 'aspect_ratios': [[1, 1], [1, 2], [2, 1]], 'scales': [1.0, 1.26, 1.59],
        'min_positive_iou': 0.5, 'max_negative_iou': 0.4}


def ground_truth(hw, g, seed):
    rng = np.random.default_rng(seed)
    y1, x1 = rng.uniform(0, 0.7 * hw[0], g), rng.uniform(0, 0.7 * hw[1], g)
    h, w = rng.uniform(12, 0.3 * hw[0], g), rng.uniform(12, 0.3 * hw[1], g)
    return (np.stack([y1, x1, y1 + h, x1 + w], 1).astype(np.float32), np.eye(8, dtype=np.float32)[rng.integers(0, 7, g)])


def run_case(hw, g, batch, rounds, steps):
    frames = synthetic.make_frames(batch, hw[0], hw[1], seed=5)
    gt = [ground_truth(hw, g, 7 + b) for b in range(batch)]
    boxes, classes = [b for b, _ in gt], [c for _, c in gt]

    def host_targets():
        samples = [create_sample_dict(frames[b], ACFG, boxes[b], classes[b]) for b in range(batch)]
        st = lambda k: np.stack([s[k] for s in samples])
        return (st(constants.ANCHORS_CLASS_TARGETS_KEY), st(constants.ANCHORS_BOX_TARGETS_KEY),
                st(constants.POSITIVE_ANCHORS_MASK_KEY), st(constants.NEGATIVE_ANCHOR_MASK_KEY)), samples[0][constants.ANCHORS_KEY]
    dense, anchors = host_targets()
    try:
        eng = Engine(make_config(hw, batch=batch, mc_samples=1, training=True))
    except MemoryError as e:
        print("%dx%d batch %d: the training handle does not fit: %s" % (hw[0], hw[1], batch, e), flush=True)
        return None
    eng.load_weights(synthetic.make_weights())
    eng.set_anchors(np.asarray(anchors, np.float32))
    eng.upload_images(frames)
    target_mb = sum(a.nbytes for a in dense) / 1e6
    counter = [0]

    def leg_a():
        counter[0] += 1
        return eng.train_step(None, *dense, seed=1, first_image_id=counter[0] * batch)

    def leg_b():
        counter[0] += 1
        return eng.train_step_boxes(None, boxes, classes, ACFG['min_positive_iou'], ACFG['max_negative_iou'], seed=1,
                                    first_image_id=counter[0] * batch)
    for _ in range(3):                                # both routes warm (first launches load code objects, set attributes)
        leg_a()
        leg_b()
    eng.synchronize()
    med = {"A": [], "B": [], "A-host": []}
    for r in range(rounds):
        for name, leg in (("A", leg_a), ("B", leg_b)) if r % 2 == 0 else (("B", leg_b), ("A", leg_a)):
            times = []
            for _ in range(steps):
                t0 = time.perf_counter()
                out = leg()                           # returns after the out6 read-back: the stream is synchronised
                times.append(time.perf_counter() - t0)
            assert np.isfinite(out["total_loss"])
            med[name].append(float(np.median(times)) * 1e3)
        t0 = time.perf_counter()
        host_targets()
        med["A-host"].append((time.perf_counter() - t0) * 1e3)
    stat = {k: (float(np.median(v)), float(max(v) - min(v))) for k, v in med.items()}
    print("%dx%d batch %d, %d boxes per frame, A = %d anchors, dense targets %.2f MB per step, %d rounds x %d steps (ms per step: "
          "median of the round medians, spread = max - min of them)" % (hw[0], hw[1], batch, g, anchors.shape[0], target_mb, rounds, steps))
    for k in ("A", "B", "A-host"):
        print("  %-7s %8.3f ms   spread %.3f ms   rounds %s" % (k, stat[k][0], stat[k][1], " ".join("%.3f" % v for v in med[k])))
    ok = stat["B"][0] <= stat["A"][0] + stat["A"][1]
    print("  B - A = %+.3f ms; B <= A + spread(A): %s; device bytes %.2f GB" % (stat["B"][0] - stat["A"][0], "yes" if ok else "NO",
                                                                               eng.device_bytes / 1e9), flush=True)
    eng.close()
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=3)
    ap.add_argument("--cases", type=str, default="512x512x5,720x1280x30", help="HxWxG, comma separated")
    args = ap.parse_args()
    results = []
    for case in args.cases.split(","):
        h, w, g = (int(v) for v in case.split("x"))
        results.append(run_case((h, w), g, args.batch, args.rounds, args.steps))
    return 0 if all(r is not False for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
