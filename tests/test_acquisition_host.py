"""Host side of the acquisition scores: the float64 reference on a record computed by hand, the ranking and the
selection of acquisition.py, and the select_frames command line through an .npz."""
import math

import numpy as np
import pytest

import acquisition_reference as ref

LN2 = math.log(2.0)
NAN = float("nan")


def _hand_record():
    """2 frames x 5 anchors, C = 4 (background last), K = 2.  Frame 0: anchors 0, 1, 4 in W, anchor 2 background, anchor 3 bad (a
    NaN co-moment).  Frame 1: every anchor background, so W is empty."""
    cls = np.zeros((2, 5, 4), np.float32)
    box = np.zeros((2, 5, 16), np.float32)
    cov = np.zeros((2, 5, 10), np.float32)
    ent = np.zeros((2, 5), np.float32)
    box[:, :, 2:4] = 1.0
    cls[1, :, 3] = 2.0
    # anchor 0: p = (.5, 0, 0, .5): H = ln 2, Ha = 0, MI = ln 2, fg = .5; e_box = (10+5+5+5) / 1 / (9+16) = 1; lda = 4 / 2 = 2; class 0
    cls[0, 0] = [1, 0, 0, 1]
    box[0, 0, 2:4] = [3, 4]
    box[0, 0, [4, 6, 9, 13]] = [10, 5, 5, 5]
    cov[0, 0, [0, 4, 5, 9]] = 1
    # anchor 1: p = (0, 1, 0, 0): H = 0, Ha = .25, MI = max(-.25, 0) = 0, fg = 1; e_box = .5 / 1 / 1 = .5; lda = -2 / 2 = -1; class 1
    cls[0, 1] = [0, 2, 0, 0]
    ent[0, 1] = 0.5
    box[0, 1, 2:4] = [1, 0]
    box[0, 1, 4] = 0.5
    cov[0, 1, 9] = -2
    # anchor 2: background (bg = 2 > thr): good, fg = 0, MI = 0: it enters mi_soft with weight 0 and nothing else
    cls[0, 2] = [0, 0, 0, 2]
    # anchor 3: bad
    cls[0, 3] = [2, 0, 0, 0]
    box[0, 3, 5] = np.nan
    # anchor 4: p = (.25, .25, 0, .5): H = 1.5 ln 2, Ha = .5 ln 2, MI = ln 2, fg = .5; e_box = 4 / 1 / 4 = 1; lda = 2 / 2 = 1; class 0
    cls[0, 4] = [0.5, 0.5, 0, 1]                          # (the first maximum wins)
    ent[0, 4] = LN2
    box[0, 4, 2:4] = [0, 2]
    box[0, 4, [4, 6, 9, 13]] = 1
    cov[0, 4, 0] = 2
    return cls, box, cov, ent


def test_reference_on_a_hand_computed_record():
    cls, box, cov, ent = _hand_record()
    thr = ref.threshold(0.5, 2)
    assert thr == np.float32(1.0)
    scores, per_class, mi = ref.acquisition(cls, box, cov, ent, 2, thr, top_k=4)       # top_k > n_fg = 3
    ln2f = float(np.float32(LN2))                          # (ent_sum is a float32)
    want0 = [3, 1, 2.5 * LN2 / 3, (0.25 + 0.5 * ln2f) / 3, (LN2 + 1.5 * LN2 - 0.5 * ln2f) / 3, LN2, LN2 / 2, 2 * LN2 / 3,
             2.5 / 3, 1.0, 2.0 / 3, 2.0]
    np.testing.assert_allclose(scores[0], want0, rtol=0, atol=1e-7)
    assert scores[1, 0] == 0 and scores[1, 1] == 0 and np.all(np.isnan(scores[1, 2:]))
    np.testing.assert_allclose(per_class[0, :2], [[2, LN2, 1.0], [1, 0.0, 0.5]], rtol=0, atol=1e-7)
    assert per_class[0, 2, 0] == 0 and np.all(np.isnan(per_class[0, 2, 1:]))
    assert np.all(per_class[1, :, 0] == 0) and np.all(np.isnan(per_class[1, :, 1:]))
    np.testing.assert_allclose(mi[0, [0, 1, 4]], [LN2, 0.0, LN2], rtol=0, atol=1e-7)
    assert np.all(np.isnan(mi[0, [2, 3]])) and np.all(np.isnan(mi[1]))
    # top_k below n_fg: the largest ones only
    assert abs(ref.acquisition(cls, box, cov, ent, 2, thr, top_k=1)[0][0, 7] - LN2) < 1e-7
    assert abs(ref.acquisition(cls, box, cov, ent, 2, thr, top_k=2)[0][0, 7] - LN2) < 1e-7
    # without ent_sum / cov_sum: exactly the MI columns / the aleatoric columns are NaN, the rest as before
    no_ent, pc_ne, mi_ne = ref.acquisition(cls, box, cov, None, 2, thr, top_k=4)
    assert np.all(np.isnan(no_ent[0, 3:8])) and np.all(np.isnan(pc_ne[:, :, 1])) and np.all(np.isnan(mi_ne))
    np.testing.assert_allclose(no_ent[0, [0, 1, 2, 8, 9, 10, 11]], np.asarray(want0)[[0, 1, 2, 8, 9, 10, 11]], rtol=0, atol=1e-7)
    no_cov = ref.acquisition(cls, box, None, ent, 2, thr, top_k=4)[0]
    assert np.all(np.isnan(no_cov[0, 10:])) and not np.any(np.isnan(no_cov[0, :10]))
    # min_foreground = 0: every good anchor (bg <= K); 1: bg <= 0
    assert ref.acquisition(cls, box, cov, ent, 2, ref.threshold(0.0, 2), 4)[0][:, 0].tolist() == [4, 5]
    assert ref.acquisition(cls, box, cov, ent, 2, ref.threshold(1.0, 2), 4)[0][:, 0].tolist() == [1, 0]


def _scores(column, values):
    from bayes_od_rc_amd import acquisition
    s = np.zeros((len(values), 12))
    s[:, acquisition.column(column)] = values
    return s


def test_rank_frames():
    from bayes_od_rc_amd import acquisition
    assert len(acquisition.COLUMNS) == 12 and acquisition.COLUMNS[7] == 'mi_topk' and acquisition.COLUMNS[0] == 'n_fg'
    s = _scores('mi_mean', [0.2, NAN, 0.7, 0.2, NAN, 0.9])
    assert acquisition.rank_frames(s, 'mi_mean').tolist() == [5, 2, 0, 3, 1, 4]      # ties and NaNs by the lower index, NaN last
    assert acquisition.rank_frames(s, 4).tolist() == [5, 2, 0, 3, 1, 4]
    assert acquisition.rank_frames(_scores('mi_max', [-np.inf, NAN, np.inf]), 'mi_max').tolist() == [2, 0, 1]
    with pytest.raises(ValueError):
        acquisition.rank_frames(s, 'mi')
    with pytest.raises(ValueError):
        acquisition.rank_frames(s[:, :5], 'mi_mean')


def _six_frames():
    """Frames 0..5, two foreground classes.  per_class[f, j] = (count, mi_max, e_box max)."""
    n = NAN
    per_class = np.asarray([[[1, .9, 1], [0, n, n]],
                            [[1, .8, 1], [1, .1, 1]],
                            [[0, n, n], [1, .7, 1]],
                            [[1, .5, 1], [1, .6, 1]],
                            [[0, n, n], [0, n, n]],
                            [[1, .95, 1], [0, n, n]]], np.float64)
    return _scores('mi_topk', [.9, .8, .7, .6, NAN, .95]), per_class


def test_select_frames():
    from bayes_od_rc_amd import acquisition
    s, pc = _six_frames()
    assert acquisition.select_frames(s, pc, 'mi_topk', 3).tolist() == [5, 0, 1]
    assert acquisition.select_frames(s, pc, 'mi_topk', 100).tolist() == [5, 0, 1, 2, 3, 4]      # a budget larger than the pool
    assert acquisition.select_frames(s, pc, 'mi_topk', 0).tolist() == []
    # class 0 (held by 0 frames, lower index): 5; class 1: 2; class 0: 0; class 1: 3 (it holds both: 3 | 2); class 1: 1; class 1: none
    # left, so the plain ranking's next frame, 4
    assert acquisition.select_frames(s, pc, 'mi_topk', 6, class_balanced=True).tolist() == [5, 2, 0, 3, 1, 4]
    assert acquisition.select_frames(s, pc, 'mi_topk', 2, class_balanced=True).tolist() == [5, 2]
    # scores without MI: the box spread decides
    pc2 = pc.copy()
    pc2[:, :, 1] = NAN
    pc2[:, :, 2] = [[3, NAN], [2, 9], [NAN, 1], [7, 5], [NAN, NAN], [1, NAN]]
    assert acquisition.select_frames(s, pc2, 'mi_topk', 3, class_balanced=True).tolist() == [3, 0, 1]
    with pytest.raises(ValueError):
        acquisition.select_frames(s, pc[:4], 'mi_topk', 3, class_balanced=True)


def test_select_frames_cli_round_trip(tmp_path, capsys):
    from bayes_od_rc_amd import acquisition, select_frames
    s, pc = _six_frames()
    names = ['frame_%d' % i for i in range(6)]
    path = acquisition.save(str(tmp_path / 'acquisition.npz'), names, s, pc)
    frames, s2, pc2 = acquisition.load(path)
    assert frames == names and np.array_equal(s2, s, equal_nan=True) and np.array_equal(pc2, pc, equal_nan=True)
    out = str(tmp_path / 'list.txt')
    got = select_frames.main(['--scores', path, '--by', 'mi_topk', '--budget', '4', '--out', out])
    assert got == ['frame_5', 'frame_0', 'frame_1', 'frame_2'] and open(out).read().split('\n') == got + ['']
    select_frames.main(['--scores', path, '--budget', '6', '--class_balanced'])
    assert capsys.readouterr().out.split() == ['frame_5', 'frame_2', 'frame_0', 'frame_3', 'frame_1', 'frame_4']
    with pytest.raises(SystemExit):
        select_frames.main(['--scores', path, '--by', 'nonsense', '--budget', '1'])
