"""Scoring-rule speed, device against host (scoring_rules.py, score_kernels.hip).

Seeded pairs as in the tests (Sigma = (A A^T + 0.5 I) s, s in {1e-2, 9, 1e4}); prints one JSON line with
  * pairs/s and Gaussian samples/s of bod_score_pairs on --rows pairs of --samples samples (median of --runs calls after a
    warm-up call; host-to-device copies included, as a caller sees it),
  * the same of score_pairs_np on --host-rows of those pairs (the first and the last half of them), and the ratio,
  * the largest |device - host| / (|host| + 1) over those pairs.

    python tests/tools/bench_scores.py --rows 200000 --samples 1000 --host-rows 2000
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from bayes_od_rc_amd import engine, scoring_rules as sr  # noqa: E402


def make_pairs(n, seed=0):
    rng = np.random.default_rng(seed)
    a = rng.normal(size=(n, 4, 4))
    s = np.array([1e-2, 9.0, 1e4])[np.arange(n) % 3]
    covs = (a @ np.transpose(a, (0, 2, 1)) + 0.5 * np.eye(4)) * s[:, None, None]
    means = rng.uniform(50.0, 900.0, size=(n, 4))
    targets = means + rng.uniform(-3.0, 3.0, size=(n, 4)) * np.sqrt(covs[:, np.arange(4), np.arange(4)])
    return means, covs, targets


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--rows', type=int, default=200000)
    ap.add_argument('--samples', type=int, default=1000)
    ap.add_argument('--host-rows', type=int, default=2000)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--device', type=int, default=0)
    args = ap.parse_args(argv)
    means, covs, targets = make_pairs(args.rows)
    engine.score_pairs(means[:1024], covs[:1024], targets[:1024], args.samples, device=args.device)          # warm-up (module load)
    times = []
    for _ in range(args.runs):
        t0 = time.perf_counter()
        out, status = engine.score_pairs(means, covs, targets, args.samples, seed=1, device=args.device)
        times.append(time.perf_counter() - t0)
    dev_s = float(np.median(times))
    k = min(args.host_rows, args.rows)
    head, tail = slice(0, k - k // 2), slice(args.rows - k // 2, args.rows)
    t0 = time.perf_counter()
    want = np.concatenate([sr.score_pairs_np(means[sl], covs[sl], targets[sl], args.samples, seed=1, first_row_id=sl.start)[0]
                           for sl in (head, tail)])
    host_s = time.perf_counter() - t0
    got = np.concatenate([out[head], out[tail]])
    dev_rate, host_rate = args.rows / dev_s, k / host_s
    row = {'rows': args.rows, 'samples': args.samples, 'device_s': [round(t, 4) for t in times], 'device_pairs_per_s': round(dev_rate, 1),
           'device_samples_per_s': round(dev_rate * args.samples, 1), 'host_rows': k, 'host_s': round(host_s, 4),
           'host_pairs_per_s': round(host_rate, 1), 'device_over_host': round(dev_rate / host_rate, 1), 'status_nonzero': int(np.sum(status != 0)),
           'max_deviation': float(np.max(np.abs(got - want) / (np.abs(want) + 1.0)))}
    print(json.dumps(row), flush=True)
    return row


if __name__ == '__main__':
    main()
