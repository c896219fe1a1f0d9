"""CPU: bench.py --dump-outputs' helpers -- padded detections with the rows past each frame's count zeroed, the packed-record form
of the N > 1 path giving the same arrays, and the 64 MB budget (a fixed sample of frames, then of MC samples)."""
import glob
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _host(b, k=100, c=8, seed=1):
    rng = np.random.default_rng(seed)
    return {"num": rng.integers(0, k + 1, b).astype(np.int32), "scores": rng.random((b, k, c), dtype=np.float32),
            "means": rng.random((b, k, 4), dtype=np.float32), "covs": rng.random((b, k, 4, 4), dtype=np.float32),
            "counts": rng.random((b, k, c), dtype=np.float32)}


def _bytes(d):
    return sum(os.path.getsize(f) for f in glob.glob(os.path.join(d, "*.npy")))


def test_detections_padding_is_zeroed_and_records_agree():
    import torch
    import bench
    from bayes_od_rc_amd import distributed as bdist
    host = _host(16)
    a = bench.detections_to_arrays(host)
    for i in range(16):
        k = host["num"][i]
        for name in ("scores", "means", "covs", "counts"):
            assert np.array_equal(a[name][i, :k], host[name][i, :k]) and not a[name][i, k:].any()
    assert np.array_equal(a["num_detections"], host["num"].astype(np.float32))
    rec = bdist.pack_records(*(torch.from_numpy(host[n]) for n in ("num", "scores", "means", "covs", "counts")))
    b = bench.records_to_arrays(rec.numpy(), 8)
    assert sorted(a) == sorted(b)
    for name in a:
        assert np.array_equal(a[name], b[name]), name


def test_dump_fits_the_budget_with_a_fixed_sample(tmp_path):
    import torch
    import bench
    a = bench.detections_to_arrays(_host(512))
    r = bench.dump_outputs(str(tmp_path / "all"), a)
    assert r["frames"] == r["of"] == 512
    for name, v in a.items():
        got = np.load(str(tmp_path / "all" / (name + ".npy")))
        assert got.dtype == np.float32 and np.array_equal(got, v)
    big = {k: np.repeat(v, 12, axis=0) for k, v in a.items()}          # 6144 frames: over 64 MB
    r1 = bench.dump_outputs(str(tmp_path / "s1"), big)
    r2 = bench.dump_outputs(str(tmp_path / "s2"), big)
    assert 0 < r1["frames"] < 6144 and _bytes(str(tmp_path / "s1")) <= 64e6
    idx = np.load(str(tmp_path / "s1" / "frame_index.npy")).astype(np.int64)
    assert np.array_equal(idx, np.load(str(tmp_path / "s2" / "frame_index.npy"))) and np.all(np.diff(idx) > 0)
    assert np.array_equal(np.load(str(tmp_path / "s1" / "covs.npy")), big["covs"][idx])
    # raw head outputs [B,N,A,.] whose single frame is over the budget: frame 0's first MC samples
    raw = {"cls": torch.ones(2, 30, 90000, 8), "box": torch.ones(2, 30, 90000, 4), "cov": torch.ones(2, 30, 90000, 10)}
    r = bench.dump_outputs(str(tmp_path / "raw"), raw)
    assert r["frames"] == 1 and 1 <= r["mc_samples"] < 30 and _bytes(str(tmp_path / "raw")) <= 64e6
    assert np.load(str(tmp_path / "raw" / "cov.npy")).shape == (1, r["mc_samples"], 90000, 10)
