#!/usr/bin/env python3
"""Measurements of profiles/acquisition_ab.txt (python tests/tools/bench_acquisition.py): bod_stat_acquisition at 512x512 for B = 64
and B = 512, with and without ent_sum: one warm-up call, then three calls; the median is reported.

Two clocks.  This script's own is the host clock around the call, which ends in the call's synchronise and its copy of B * 33 doubles:
an upper bound that includes a launch, a copy and a synchronise.  The time on the stream is the two kernels' own, read from a kernel
trace of this same script (one run of its own, the dispatches in the order printed here):
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tests/tools/bench_acquisition.py
Each figure stands beside the byte floor of the streaming pass, B * A * (C + 16 + 10 + 1) * 4 bytes at the 8.0 TB/s HBM3E peak and at
the 6.3 TB/s a float4 copy achieves on the chip, and beside stat_merge_kernel's time for the same B (profiles/stat_merge_ab.txt)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
from bayes_od_rc_amd.engine import Engine, make_config

HBM_PEAK_TBS, HBM_COPY_TBS = 8.0, 6.3
# profiles/stat_merge_ab.txt (b): measured at B = 512 only (1.783 ms for 10.26 GB); its B = 64 figure is that file's own scaling
STAT_MERGE_MS = {512: "1.783 ms measured", 64: "about 0.2 ms (scaled from B = 512 there, not measured)"}
hw, C, K = (512, 512), 8, 10


def one_frame_record(a_n, seed=5, bias=9.0):
    """One frame's fp32 record of K random samples per anchor, the background logit biased so that a minority is foreground."""
    rng = np.random.default_rng(seed)
    logits = rng.normal(0, 2.0, (K, a_n, C))
    logits[..., C - 1] += bias
    p = np.exp(logits - logits.max(axis=2, keepdims=True))
    p /= p.sum(axis=2, keepdims=True)
    box = np.zeros((a_n, 16))
    box[:, :4] = rng.uniform(8.0, 400.0, (a_n, 4))
    box[:, [4, 6, 9, 13]] = rng.uniform(0.5, 20.0, (a_n, 4))
    f32 = lambda v: np.ascontiguousarray(v[None], np.float32)
    return f32(p.sum(axis=0)), f32(box), f32(rng.normal(0, 1.0, (a_n, 10))), f32(-(p * np.log(p)).sum(axis=2).sum(axis=0))


for B in (64, 512):
    for ent in (True, False):
        eng = Engine(make_config(hw, batch=B, mc_samples=2, mc_statistics=True, class_parts=ent))
        rec = [np.ascontiguousarray(np.broadcast_to(v, (B,) + v.shape[1:])) for v in one_frame_record(eng.A)]      # the same frame B times
        eng.set_statistics(rec[0], rec[1], rec[2], samples=K)
        if ent:
            eng.set_entropy(rec[3])
        del rec
        scores, _ = eng.stat_acquisition()                           # warm-up (allocates the scratch)
        times = []
        for _ in range(3):
            eng.synchronize()
            t0 = time.perf_counter()
            eng.stat_acquisition()
            times.append((time.perf_counter() - t0) * 1e3)
        byts = 4.0 * B * eng.A * (C + 16 + 10 + 1)
        ms = float(np.median(times))
        print("bod_stat_acquisition B=%d A=%d ent_sum=%d (n_fg %d of %d per frame): host clock median %.3f ms of [%s]; pass reads %.2f GB: "
              "byte floor %.3f ms at %.1f TB/s, %.3f ms at %.1f TB/s; stat_merge_kernel at this B: %s"
              % (B, eng.A, ent, scores[0, 0], eng.A, ms, " ".join("%.3f" % t for t in times), byts / 1e9, byts / (HBM_PEAK_TBS * 1e9),
                 HBM_PEAK_TBS, byts / (HBM_COPY_TBS * 1e9), HBM_COPY_TBS, STAT_MERGE_MS[B]), flush=True)
        eng.close()
