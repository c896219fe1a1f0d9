"""GPU: the scoring rules on the device (score_kernels.hip: bod_score_pairs) against their host statement
(bayes_od_rc_amd/scoring_rules.py: score_pairs_np, pinned to scipy / numpy.linalg by test_scoring_rules_host.py).

Both sides are fp64 on the same Philox words; they differ by a few ulp of the device's log, sincos and erfc and by the
order of sums of at most 65 536 terms, which the subtraction in the energy score and the near-tail PIT values amplify by at
most a few hundred: every column of every row agrees within 1e-9 (|want| + 1).  A row's bits depend on its id alone."""
import functools

import numpy as np
import pytest

from bayes_od_rc_amd import engine, scoring_rules as sr

import scores_reference as ref

pytestmark = pytest.mark.gpu

N_MAX = 257
SEED = 0x1234567890ABCDEF
FIRST = (1 << 32) - 100            # the ids of the 257 rows cross the 32-bit boundary of the counter's two row words
MEANS, COVS, TARGETS = ref.pd_pairs(N_MAX)


@functools.lru_cache(maxsize=None)
def _want(m):
    out, status = sr.score_pairs_np(MEANS, COVS, TARGETS, num_samples=m, seed=SEED, first_row_id=FIRST)
    assert not status.any()
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _got(n, m):
    out, status = engine.score_pairs(MEANS[:n], COVS[:n], TARGETS[:n], num_samples=m, seed=SEED, first_row_id=FIRST, device=0)
    out.setflags(write=False)
    return out, status


@pytest.mark.parametrize("m", [2, 63, 64, 65, 1000])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 64, 257])
def test_every_column_agrees_with_the_host(n, m):
    got, status = _got(n, m)
    want = _want(m)[:n]
    assert got.shape == (n, 8) and status.shape == (n,) and not status.any()
    dev = np.abs(got - want) / (np.abs(want) + 1.0)
    print("n=%d M=%d: largest deviation per column %s" % (n, m, " ".join("%.2e" % v for v in dev.max(axis=0))))
    assert np.isfinite(got).all()
    assert (dev <= 1e-9).all(), (np.argwhere(dev > 1e-9)[:5], float(dev.max()))


def test_bits_are_repeatable_and_belong_to_the_row():
    batch, _ = _got(N_MAX, 1000)
    again, _ = engine.score_pairs(MEANS, COVS, TARGETS, num_samples=1000, seed=SEED, first_row_id=FIRST, device=0)
    assert batch.tobytes() == again.tobytes()
    for k in (0, 99, 100, 130, 256):                # (ids 2^32 - 1 and 2^32 are rows 99 and 100)
        alone, status = engine.score_pairs(MEANS[k], COVS[k], TARGETS[k], num_samples=1000, seed=SEED, first_row_id=FIRST + k, device=0)
        assert status[0] == 0 and alone[0].tobytes() == batch[k].tobytes(), k
    # the upper triangle is not read
    junk = COVS[:5].copy()
    junk[:, np.triu_indices(4, 1)[0], np.triu_indices(4, 1)[1]] = np.nan
    out, status = engine.score_pairs(MEANS[:5], junk, TARGETS[:5], num_samples=1000, seed=SEED, first_row_id=FIRST, device=0)
    assert not status.any() and out.tobytes() == batch[:5].tobytes()


def test_bad_rows_are_marked_and_disturb_nothing():
    means, covs, targets = MEANS[:6].copy(), COVS[:6].copy(), TARGETS[:6].copy()
    covs[1, 2, 1] = np.inf
    covs[4] = np.diag([1.0, 1.0, -1.0, 1.0])
    out, status = engine.score_pairs(means, covs, targets, num_samples=65, seed=SEED, first_row_id=40, device=0)
    assert status.tolist() == [0, 2, 0, 0, 1, 0]
    assert np.isnan(out[[1, 4]]).all()
    for k in (0, 2, 3, 5):
        alone, st = engine.score_pairs(means[k], covs[k], targets[k], num_samples=65, seed=SEED, first_row_id=40 + k, device=0)
        assert st[0] == 0 and alone[0].tobytes() == out[k].tobytes(), k
    want, want_status = sr.score_pairs_np(means, covs, targets, num_samples=65, seed=SEED, first_row_id=40)
    assert want_status.tolist() == status.tolist()


def test_arguments():
    out, status = engine.score_pairs(np.zeros((0, 4)), np.zeros((0, 4, 4)), np.zeros((0, 4)), device=0)
    assert out.shape == (0, 8) and status.shape == (0,)
    for bad in (1, 65537):
        with pytest.raises(ValueError, match="num_samples"):
            engine.score_pairs(MEANS[:2], COVS[:2], TARGETS[:2], num_samples=bad, device=0)
    out, status = engine.score_pairs(MEANS[:2], COVS[:2], TARGETS[:2], num_samples=65536, seed=SEED, first_row_id=FIRST, device=0)
    want, _ = sr.score_pairs_np(MEANS[:2], COVS[:2], TARGETS[:2], num_samples=65536, seed=SEED, first_row_id=FIRST)
    assert not status.any() and (np.abs(out - want) <= 1e-9 * (np.abs(want) + 1.0)).all()


def test_report_on_the_device_equals_the_host_report(tmp_path):
    gt, root = ref.write_tree(str(tmp_path))
    host = sr.scores_report(gt, root, ref.TREE_FRAMES, num_samples=1000, seed=5, parts=True)
    dev = sr.scores_report(gt, root, ref.TREE_FRAMES, num_samples=1000, seed=5, parts=True, device=0)
    for k, v in ref.TREE_COUNTS.items():
        assert dev[k] == v

    def same(a, b, path):
        assert type(a) is type(b), path
        if isinstance(a, dict):
            assert a.keys() == b.keys(), path
            for k in a:
                same(a[k], b[k], path + "." + k)
        elif isinstance(a, float):
            assert abs(a - b) <= 1e-9 * abs(b), (path, a, b)
        else:
            assert a == b, (path, a, b)

    same(dev, host, "report")
