"""CPU: the host side of the scoring rules (bayes_od_rc_amd/scoring_rules.py): its Philox against the oracle's, nll / PIT /
Mahalanobis / ln det against scipy and numpy.linalg, the energy score's definition pinned four ways, the greedy matching
against evaluation_utils_2d._match, and the report on a small tree with hand-computed counts."""
import json
import math

import numpy as np
import pytest

from bayes_od_rc_amd import evaluation_utils_2d as ev, offline_eval, scoring_rules as sr
from oracle import philox as oracle_philox

import scores_reference as ref


def _close(got, want, rtol=1e-12):
    np.testing.assert_allclose(got, want, rtol=rtol, atol=0)


# the Gaussian of the energy-score checks: a box of ordinary size, a few pixels off
def _es_case():
    rng = np.random.default_rng(1)
    a = rng.normal(size=(4, 4))
    cov = (a @ a.T + 0.5 * np.eye(4)) * 9.0
    mu = np.array([300.0, 640.0, 80.0, 120.0])
    return mu, cov, mu + np.array([3.0, -2.0, 5.0, 1.0])


def _es_terms(mu, cov, g, normals):
    z = mu + normals @ np.linalg.cholesky(cov).T
    return np.linalg.norm(z - g, axis=1), np.linalg.norm(z[:-1] - z[1:], axis=1)


def test_philox_equals_the_oracle_word_for_word():
    rng = np.random.default_rng(0)
    c = rng.integers(0, 2 ** 32, size=(4, 1000), dtype=np.uint64)
    for k0, k1 in ((0, 0), (0xDEADBEEF, 0x12345678), (0xFFFFFFFF, 0xFFFFFFFF)):
        got = sr.philox4x32_10(c[0], c[1], c[2], c[3], k0, k1)
        want = oracle_philox.philox4x32_10(c[0], c[1], c[2], c[3], k0, k1)
        for a, b in zip(got, want):
            assert a.dtype == np.uint32 and np.array_equal(a, b)


def test_closed_form_columns_against_independent_code():
    from scipy.stats import multivariate_normal, norm
    means, covs, targets = ref.pd_pairs(40)
    out, status = sr.score_pairs_np(means, covs, targets, num_samples=2)
    assert not status.any()
    for i in range(len(means)):
        _close(out[i, 0], -multivariate_normal.logpdf(targets[i], means[i], covs[i]))
        d = targets[i] - means[i]
        _close(out[i, 1], d @ np.linalg.solve(covs[i], d))
        _close(out[i, 3:7], norm.cdf(d / np.sqrt(np.diag(covs[i]))))
        _close(out[i, 7], np.linalg.slogdet(covs[i])[1])
    # the upper triangle is not read
    junk = covs.copy()
    junk[:, np.triu_indices(4, 1)[0], np.triu_indices(4, 1)[1]] = np.nan
    out2, status2 = sr.score_pairs_np(means, junk, targets, num_samples=2)
    assert not status2.any() and np.array_equal(out, out2)


@pytest.mark.parametrize("m", [2, 63, 64, 65, 1000])
def test_energy_score_equals_a_plain_loop(m):
    mu, cov, g = _es_case()
    seed, row = 12345, (5 << 32) + 7
    n = sr.score_normals([row], m, seed)[0]
    L = np.linalg.cholesky(cov)
    z = [mu + L @ n[i] for i in range(m)]
    s_a = sum(math.sqrt(sum((z[i][k] - g[k]) ** 2 for k in range(4))) for i in range(m))
    s_b = sum(math.sqrt(sum((z[i][k] - z[i + 1][k]) ** 2 for k in range(4))) for i in range(m - 1))
    out, status = sr.score_pairs_np(mu, cov, g, num_samples=m, seed=seed, first_row_id=row)
    assert status[0] == 0
    _close(out[0, 2], s_a / m - s_b / (2 * (m - 1)))


def test_normals_follow_the_contract():
    """One sample spelled out: a single Philox call, u = (t + 0.5) 2^-32, two Box-Muller pairs."""
    seed, row, i = (9 << 32) + 4, (3 << 32) + 11, 17
    w = [int(t) for t in oracle_philox.philox4x32_10(i, row & 0xFFFFFFFF, 0x005C04E5, row >> 32, seed & 0xFFFFFFFF, seed >> 32)]
    u = [(t + 0.5) * 2.0 ** -32 for t in w]
    want = [math.sqrt(-2 * math.log(u[0])) * math.cos(2 * math.pi * u[1]), math.sqrt(-2 * math.log(u[0])) * math.sin(2 * math.pi * u[1]),
            math.sqrt(-2 * math.log(u[2])) * math.cos(2 * math.pi * u[3]), math.sqrt(-2 * math.log(u[2])) * math.sin(2 * math.pi * u[3])]
    _close(sr.score_normals([row], 32, seed)[0, i], want, rtol=1e-13)


def test_energy_score_of_a_point_mass_is_the_distance():
    mu, cov, g = _es_case()
    out, _ = sr.score_pairs_np(mu, cov * 1e-12, g, num_samples=1000)
    assert abs(out[0, 2] - np.linalg.norm(mu - g)) < 1e-4


def test_energy_score_within_five_standard_errors_of_independent_normals():
    """M = 65 536 contract normals against the same estimator on numpy's generator.  Both estimates carry the standard error
    sqrt(var(|z - g|) / M + var(|z - z'|) / (4 (M - 1))); their difference sqrt(2) times it.  Fixed seeds: deterministic."""
    mu, cov, g = _es_case()
    m = 65536
    out, _ = sr.score_pairs_np(mu, cov, g, num_samples=m, seed=12345, first_row_id=7)
    a, b = _es_terms(mu, cov, g, sr.score_normals([7], m, 12345)[0])
    _close(out[0, 2], a.sum() / m - b.sum() / (2 * (m - 1)))
    a2, b2 = _es_terms(mu, cov, g, np.random.default_rng(0).standard_normal((m, 4)))
    other = a2.sum() / m - b2.sum() / (2 * (m - 1))
    se = math.sqrt(a.var() / m + b.var() / (4 * (m - 1))) * math.sqrt(2.0)
    print("energy score %.6f, independent %.6f, difference %.4g, 5 se %.4g" % (out[0, 2], other, abs(out[0, 2] - other), 5 * se))
    assert abs(out[0, 2] - other) < 5 * se


def test_a_row_depends_on_its_id_alone():
    means, covs, targets = ref.pd_pairs(9)
    alone, _ = sr.score_pairs_np(means[:1], covs[:1], targets[:1], num_samples=100, seed=3, first_row_id=1000)
    more, _ = sr.score_pairs_np(means, covs, targets, num_samples=100, seed=3, first_row_id=1000)
    assert np.array_equal(alone[0], more[0])
    # placed fifth in a call that starts four ids lower
    shifted, _ = sr.score_pairs_np(np.roll(means, 4, 0), np.roll(covs, 4, 0), np.roll(targets, 4, 0), num_samples=100, seed=3, first_row_id=996)
    assert np.array_equal(alone[0], shifted[4])
    other, _ = sr.score_pairs_np(means[:1], covs[:1], targets[:1], num_samples=100, seed=3, first_row_id=1001)
    assert other[0, 2] != alone[0, 2] and np.array_equal(other[0, [0, 1, 3, 4, 5, 6, 7]], alone[0, [0, 1, 3, 4, 5, 6, 7]])
    # a chunk boundary inside the call changes nothing
    old = sr._CHUNK_SAMPLES
    try:
        sr._CHUNK_SAMPLES = 250
        chunked, _ = sr.score_pairs_np(means, covs, targets, num_samples=100, seed=3, first_row_id=1000)
    finally:
        sr._CHUNK_SAMPLES = old
    assert np.array_equal(chunked, more)


def test_status_and_arguments():
    means, covs, targets = ref.pd_pairs(6)
    covs[1, 2, 1] = np.inf                                   # lower triangle: read
    covs[4] = np.diag([1.0, 1.0, -1.0, 1.0])
    means[5, 0] = np.nan
    out, status = sr.score_pairs_np(means, covs, targets, num_samples=16)
    assert status.tolist() == [0, 2, 0, 0, 1, 2]
    assert np.isnan(out[[1, 4, 5]]).all() and np.isfinite(out[[0, 2, 3]]).all()
    for k in (0, 2, 3):
        alone, _ = sr.score_pairs_np(means[k], covs[k], targets[k], num_samples=16, first_row_id=k)
        assert np.array_equal(alone[0], out[k])
    out0, status0 = sr.score_pairs_np(np.zeros((0, 4)), np.zeros((0, 4, 4)), np.zeros((0, 4)))
    assert out0.shape == (0, 8) and status0.shape == (0,)
    for bad in (1, 65537):
        with pytest.raises(ValueError):
            sr.score_pairs_np(means, covs, targets, num_samples=bad)


def test_match_frame_marks_what_ev_match_marks():
    gt = [[0, 0, 9, 9], [20, 0, 39, 19], [100, 100, 119, 119]]
    det = [[0, 0, 9, 4],          # IoU with gt 0 = 50 / 100: exactly the threshold -> false positive
           [21, 0, 39, 19],       # gt 1
           [20, 1, 39, 19],       # gt 1 again: taken -> false positive
           [0, 0, 9, 8],          # gt 0 (0.9), still free
           [200, 200, 210, 210]]  # nothing
    order = [0, 1, 2, 3, 4]
    pairs, fps, fns = sr.match_frame(gt, det, order, 0.5)
    assert pairs == [(1, 1), (3, 0)] and fps == [0, 2, 4] and fns == [2]
    tp, fp, _ = ev._match([{'name': 'f', 'bbox': b} for b in gt], [{'name': 'f', 'bbox': det[d]} for d in order], [0.5])
    assert [order[i] for i in np.nonzero(tp[:, 0])[0]] == [d for d, _ in pairs]
    assert [order[i] for i in np.nonzero(fp[:, 0])[0]] == fps
    # another order: the later claimant of gt 1 now wins
    pairs2, fps2, _ = sr.match_frame(gt, det, [2, 1, 3], 0.5)
    assert pairs2 == [(2, 1), (3, 0)] and fps2 == [1]
    assert sr.match_frame(np.zeros((0, 4)), det, order, 0.5) == ([], order, [])


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return ref.write_tree(str(tmp_path_factory.mktemp("scores_tree")))


def test_scores_report_on_a_hand_made_tree(tree):
    gt, root = tree
    rep = sr.scores_report(gt, root, ref.TREE_FRAMES, num_samples=64, seed=5, parts=True)
    for k, v in ref.TREE_COUNTS.items():
        assert rep[k] == v, k
    # the four scored pairs, rebuilt by hand: frame a detections 0, 2; frame c detections 2, 0 (score order)
    T = np.array([[0, 1, 0, -0.5], [1, 0, -0.5, 0], [0, 1, 0, 0.5], [1, 0, 0.5, 0]])
    rows = []
    for fi, name, d, box in ((0, 'a', 0, gt[0]['bbox']), (0, 'a', 2, gt[1]['bbox']), (2, 'c', 2, gt[6]['bbox']), (2, 'c', 0, gt[5]['bbox'])):
        mean = np.load("%s/mean/%s.npy" % (root, name)).astype(np.float64)[d]
        cov = np.load("%s/cov/%s.npy" % (root, name)).astype(np.float64)[d]
        o, s = sr.score_pairs_np(T @ mean, T @ cov @ T.T, box, num_samples=64, seed=5, first_row_id=fi * 65536 + d)
        assert s[0] == 0
        rows.append(o[0])
    rows = np.array(rows)
    _close(rep['mean_nll'], rows[:, 0].mean())
    _close(rep['median_nll'], np.median(rows[:, 0]))
    _close(rep['mean_energy_score'], rows[:, 2].mean())
    _close(rep['mean_mahalanobis2'], rows[:, 1].mean())
    _close(rep['fitted_cov_scale'], rows[:, 1].mean() / 4)
    s = rep['fitted_cov_scale']
    _close(rep['nll_at_fitted_scale'], np.mean(0.5 * (4 * math.log(2 * math.pi) + rows[:, 7] + 4 * math.log(s) + rows[:, 1] / s)))
    assert rep['nll_at_fitted_scale'] <= rep['mean_nll']
    qs = np.arange(1, 10) / 10
    _close(rep['calibration_error'], np.mean([[abs(np.mean(rows[:, 3 + k] <= q) - q) for q in qs] for k in range(4)]))
    # classification: true positives a0 (car 0.90 on a car), a2 (rider 0.70 on a person), a6 (bus 0.66), c2 (0.90), c0 (0.85)
    cats = {n: np.load("%s/cat_param/%s.npy" % (root, n)).astype(np.float64) for n in 'ac'}
    tp = [(cats['a'][0], 0), (cats['a'][2], 3), (cats['a'][6], 2), (cats['c'][2], 0), (cats['c'][0], 0)]
    _close(rep['cls_nll'], np.mean([-math.log(p[c] / p.sum()) for p, c in tp]))
    _close(rep['brier'], np.mean([np.sum((p / p.sum() - np.eye(8)[c]) ** 2) for p, c in tp]))
    fp = [cats['a'][1], cats['a'][3], cats['a'][5], cats['c'][1], cats['c'][4]]
    _close(rep['fp_nll'], np.mean([-math.log(p[7] / p.sum()) for p in fp]))
    # ece: bins of width 0.1; correct = true positive with the right arg-max (a2 is a true positive of the wrong class)
    conf = np.array([0.90, 0.70, 0.66, 0.90, 0.85, 0.80, 0.95, 0.60, 0.75, 0.65], np.float32).astype(np.float64)
    hit = np.array([1, 0, 1, 1, 1, 0, 0, 0, 0, 0], float)
    bins = np.minimum((conf * 10).astype(int), 9)
    _close(rep['ece'], sum(np.sum(bins == b) / 10 * abs(hit[bins == b].mean() - conf[bins == b].mean()) for b in set(bins.tolist())))
    # parts: shares 0.25 / 0.25 of cov -> m2 scales by 4 and 2, the singular pair is singular in each of them
    assert set(rep['parts']) == {'epistemic', 'aleatoric', 'epistemic+aleatoric'}
    for name, share in (('epistemic', 0.25), ('aleatoric', 0.25), ('epistemic+aleatoric', 0.5)):
        block = rep['parts'][name]
        assert block['n_singular'] == 1
        _close(block['mean_mahalanobis2'], rep['mean_mahalanobis2'] / share, rtol=1e-9)
        _close(block['nll_at_fitted_scale'], rep['nll_at_fitted_scale'], rtol=1e-9)       # the fitted scale undoes the share
    # the covariance scale is applied before scoring; without the part trees there is no parts block
    rep2 = sr.scores_report(gt, root, ref.TREE_FRAMES, num_samples=64, seed=5, cov_scale=4.0)
    assert 'parts' not in rep2 and rep2['n_singular'] == 1
    _close(rep2['mean_mahalanobis2'], rep['mean_mahalanobis2'] / 4, rtol=1e-9)
    # the report does not depend on which frames surround a frame's index: ids come from the index in `frames`
    only_c = sr.scores_report(gt, root, ['c'], num_samples=64, seed=5)
    assert (only_c['n_tp'], only_c['n_fp'], only_c['n_fn'], only_c['n_singular']) == (2, 2, 0, 0)


def test_cli_returns_the_report(tree, capsys):
    gt, root = tree
    args = ['scores', '--labels', root + '/labels.json', '--predictions', root, '--samples', '64', '--seed', '5', '--parts']
    out = offline_eval.main(args)
    assert out == sr.scores_report(gt, root, ref.TREE_FRAMES, num_samples=64, seed=5, parts=True)
    assert json.loads(capsys.readouterr().out) == out
    with pytest.raises(SystemExit, match="kitti_records"):
        offline_eval.main(args + ['--dataset', 'kitti'])
