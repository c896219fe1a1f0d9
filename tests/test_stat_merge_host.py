"""Mergeable MC statistics, host side: the ABI of the bod_stat_* entry points, the mc_statistics config field, the float64
statement of the merge formula (distributed.merge_statistics_np) and the all-gather + rank-order fold over gloo."""
import ctypes
import os
import re
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAT_SYMBOLS = ["bod_stat_device", "bod_stat_forward", "bod_stat_get", "bod_stat_merge", "bod_stat_merge_from", "bod_stat_posterior",
                "bod_stat_reset", "bod_stat_set"]


def test_stat_symbols_in_header_binding_cdef_and_library():
    from bayes_od_rc_amd import _lib, build
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bayesod.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(bod_[a-z0-9_]+)\s*\(", header))
    cdef = set(re.findall(r"\b(bod_[a-z0-9_]+)\s*\(", build.cdef_text()))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in STAT_SYMBOLS:
        assert name in declared and name in cdef and name in _lib.SIGNATURES, name
        assert getattr(lib, name) is not None
    assert open(os.path.join(ROOT, "include", "bayesod_cdef.h")).read() == build.cdef_text()
    # the field took one of the two reserved ints: size and the offsets in front of it are unchanged
    assert ctypes.sizeof(_lib.BodConfig) == 31 * 4
    assert _lib.BodConfig.mc_statistics.offset == 29 * 4 and _lib.BodConfig.pipeline_overlap.offset == 28 * 4
    assert re.search(r"int32_t\s+mc_statistics;", header) and re.search(r"int32_t\s+reserved\[1\];", header)


def test_make_config_translates_mc_statistics():
    from bayes_od_rc_amd.engine import make_config
    assert make_config((128, 128)).mc_statistics == 0
    cfg = make_config((128, 128), mc_samples=3, mc_ensemble_size=12, mc_statistics=True)
    assert cfg.mc_statistics == 1 and cfg.mc_ensemble_size == 12 and cfg.mc_samples == 3
    with pytest.raises(ValueError):
        make_config((128, 128), mc_samples=1, mc_statistics=True, training=True)
    with pytest.raises(ValueError):
        make_config((128, 128), mc_statistics=True, pipeline_overlap=True)


def _group_stats(boxes, t=np.float64):
    """Statistics record of per-sample boxes [n,A,4] (and fake class / covariance sums) in dtype t."""
    x = boxes.astype(t)
    mean = x.mean(axis=0)
    d = x - mean
    m2 = np.einsum("nai,naj->aij", d, d)
    rec = np.zeros((x.shape[1], 16), t)
    rec[:, :4] = mean
    k = 4
    for i in range(4):
        for j in range(i + 1):
            rec[:, k] = m2[:, i, j]
            k += 1
    return rec


def _fake_record(rng, boxes):
    n, a = boxes.shape[:2]
    return (rng.random((n, a, 8)).sum(axis=0), _group_stats(boxes), rng.normal(size=(n, a, 10)).sum(axis=0))


def test_merge_statistics_np_equals_the_whole_set():
    from bayes_od_rc_amd.distributed import merge_statistics_np
    rng = np.random.default_rng(5)
    a = 40
    for sizes in ((1, 4), (5, 5), (2, 7), (3, 1, 6, 2), (1, 1, 1)):
        boxes = rng.normal(50.0, 20.0, (sum(sizes), a, 4)) + rng.normal(0, 1.0, (sum(sizes), a, 4))
        cls = rng.random((sum(sizes), a, 8))
        cov = rng.normal(size=(sum(sizes), a, 10))
        acc, k, lo = None, 0, 0
        for n in sizes:
            rec = (cls[lo:lo + n].sum(axis=0), _group_stats(boxes[lo:lo + n]), cov[lo:lo + n].sum(axis=0))
            acc = merge_statistics_np(acc if acc is not None else rec, rec, k, n)
            k, lo = k + n, lo + n
        whole = _group_stats(boxes)
        scale = np.abs(whole) + 1.0
        assert np.max(np.abs(acc[1] - whole) / scale) < 1e-12
        assert np.all(acc[1][:, 14:] == 0)
        assert np.max(np.abs(acc[0] - cls.sum(axis=0))) < 1e-12 and np.max(np.abs(acc[2] - cov.sum(axis=0))) < 1e-12


def test_merge_statistics_np_ka_zero_copies_and_is_associative():
    from bayes_od_rc_amd.distributed import merge_statistics_np
    rng = np.random.default_rng(6)
    recs = [_fake_record(rng, rng.normal(10.0, 5.0, (n, 25, 4))) for n in (3, 5, 2)]
    garbage = tuple(np.full_like(x, np.nan) for x in recs[0])
    copied = merge_statistics_np(garbage, recs[1], 0, 5)
    for got, want in zip(copied, recs[1]):
        assert np.array_equal(got, want)
    left = merge_statistics_np(merge_statistics_np(recs[0], recs[1], 3, 5), recs[2], 8, 2)
    right = merge_statistics_np(recs[0], merge_statistics_np(recs[1], recs[2], 5, 2), 3, 7)
    for l, r in zip(left, right):
        assert np.max(np.abs(l - r) / (np.abs(r) + 1.0)) < 1e-12
    # without the covariance head the third array stays absent
    assert merge_statistics_np(recs[0][:2] + (None,), recs[1][:2] + (None,), 3, 5)[2] is None
    # float32: the kernel's own operation order, rounded per operation
    f32 = merge_statistics_np(recs[0], recs[1], 3, 5, dtype=np.float32)
    assert all(x.dtype == np.float32 for x in f32)


def _rank_record(rank, b=2, a=37):
    rng = np.random.default_rng(300 + rank)
    boxes = rng.normal(30.0, 10.0, (4, b * a, 4))
    cls, box, cov = _fake_record(rng, boxes)
    return {"cls": torch.from_numpy(cls.reshape(b, a, 8).astype(np.float32)),
            "box": torch.from_numpy(box.reshape(b, a, 16).astype(np.float32)),
            "cov": torch.from_numpy(cov.reshape(b, a, 10).astype(np.float32))}


def _fold(records, n):
    from bayes_od_rc_amd.distributed import merge_statistics_np
    acc, k = None, 0
    for r in records:
        rec = (r["cls"].numpy(), r["box"].numpy(), r["cov"].numpy())
        acc = merge_statistics_np(acc if acc is not None else rec, rec, k, n, dtype=np.float32)
        k += n
    return acc


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from bayes_od_rc_amd import distributed as bd
    gathered = bd.all_gather_statistics(_rank_record(rank))
    assert len(gathered) == world
    for r in range(world):                      # rank r's record arrived unchanged, every part 16-byte aligned in its buffer
        for k, v in _rank_record(r).items():
            assert torch.equal(gathered[r][k], v)
            assert gathered[r][k].data_ptr() % 16 == 0
    q.put((rank, [np.ascontiguousarray(x) for x in _fold(gathered, 4)]))
    dist.barrier()
    dist.destroy_process_group()


def test_all_gather_statistics_and_rank_order_fold_world2_gloo():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=120) for _ in range(2))
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    want = _fold([_rank_record(0), _rank_record(1)], 4)
    for r in range(2):
        for g, w in zip(got[r], want):
            assert np.array_equal(g, w)         # the same bits on both ranks, and those of the rank-order fold


def test_all_gather_statistics_single_process():
    from bayes_od_rc_amd import distributed as bd
    rec = _rank_record(0)
    out = bd.all_gather_statistics({k: rec[k] for k in ("cls", "box")})
    assert len(out) == 1 and sorted(out[0]) == ["box", "cls"] and torch.equal(out[0]["box"], rec["box"])
