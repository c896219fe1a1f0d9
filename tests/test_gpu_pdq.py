"""GPU: PDQ on the device (pdq_kernels.hip: bod_pdq_corner_heatmaps / bod_pdq_frames) against the CPU restatement
(bayes_od_rc_amd/prob_detection_quality.py, pinned to the reference by tests/golden/pdq.npz).

Heatmaps agree within 1e-6, except pixels where one side lies within 1e-6 of the 0.0027 floor and the other side floored
it (counted, asserted few).  The losses agree with a float64 sum of NumPy's float32 per-pixel terms on the device's own
heatmaps to relative 2e-7 (the reductions alone) and with the CPU path's float32 tensordots to relative 1e-5."""
import os

import numpy as np
import pytest

from bayes_od_rc_amd import engine, offline_eval, prob_detection_quality as pdq

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pdq.npz"))
SHAPE = tuple(int(v) for v in G["img_shape"])
FLOOR = pdq.HEATMAP_FLOOR


def _maps_close(got, want, tol=1e-6):
    """Number of floor-boundary pixels; asserts every other pixel agrees within tol."""
    got = np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    bad = np.abs(got - want) > tol
    excused = bad & ((got == 0) | (want == 0)) & ((np.abs(got - FLOOR) <= tol) | (np.abs(want - FLOOR) <= tol))
    assert not (bad & ~excused).any(), (np.argwhere(bad & ~excused)[:5], np.abs(got - want).max())
    return int(excused.sum())


def _golden_image(k):
    gts = []
    for b, l in zip(G["img%d_gt_boxes" % k], G["img%d_gt_labels" % k]):
        m = np.zeros(SHAPE, dtype=bool)
        m[b[1]:b[3], b[0]:b[2]] = True
        gts.append(pdq.GroundTruthInstance(m, int(l), 0, 0, bounding_box=np.array(b)))
    dets = [pdq.PBoxDetInst(G["pbox_probs"][i], G["pbox_boxes"][i], [G["pbox_covs"][i][0], G["pbox_covs"][i][1]])
            for i in G["img%d_det_idx" % k]]
    return gts, dets


def test_corner_regions_and_heatmaps():
    rois, heat = engine.pdq_corner_heatmaps(SHAPE, G["corner_means"], G["corner_covs"], device=0)
    np.testing.assert_array_equal(rois, G["corner_rois"])
    assert _maps_close(heat, G["corner_heatmaps"]) <= 2
    # and against the CPU restatement itself
    for k, (m, c) in enumerate(zip(G["corner_means"], G["corner_covs"])):
        assert _maps_close(heat[k], pdq.corner_heatmap(SHAPE, list(m), c)) <= 2


def test_box_heatmaps_of_frames():
    covs = np.asarray(G["pbox_covs"], np.float64)
    fg, bg, dbg, heat = engine.pdq_frames(SHAPE, [0], np.zeros((0, 4), np.int32), [4], G["pbox_boxes"], covs, device=0, heatmaps=True)
    assert fg[0].shape == (0, 4) and dbg[0].shape == (4,)
    for k in range(4):
        assert _maps_close(heat[k], G["pbox_heatmaps"][k]) <= 2
        assert heat[k].max() <= 1 and (heat[k][heat[k] > 0] >= FLOOR).all()


def test_golden_images_through_device_pdq():
    ev = pdq.PDQ(device=0)
    for k in range(int(G["n_images"])):
        gts, dets = _golden_image(k)
        one = pdq.PDQ(device=0)
        one.add_img_eval(gts, dets)
        want = G["image_results"][k]
        np.testing.assert_allclose([one._tot_overall_quality, one._tot_spatial_quality, one._tot_label_quality], want[:3], atol=1e-5, rtol=0)
        assert list(one.get_assignment_counts()) == [int(v) for v in want[3:]], k
    score = ev.score([_golden_image(k) for k in range(int(G["n_images"]))])
    tot = G["pdq_totals"]
    np.testing.assert_allclose([score, ev.get_avg_spatial_score(), ev.get_avg_label_score(), ev.get_avg_overall_quality_score()],
                               tot[:4], atol=1e-5, rtol=0)
    assert list(ev.get_assignment_counts()) == [int(v) for v in tot[4:]]


def _cov(rng, sx, sy):
    r = rng.uniform(-0.6, 0.6)
    return np.array([[sx * sx, r * sx * sy], [r * sx * sy, sy * sy]])


def _frames(rng, shape, n_frames, sigma, n_gt=4, n_det=4):
    """Seeded frames: boxes off every edge, a ground truth with negative coordinates, a frame without detections and one
    without ground truth."""
    h, w = shape
    out = []
    for f in range(n_frames):
        ng = 0 if f == 1 else n_gt
        nd = 0 if f == 2 else n_det
        gts = []
        for k in range(ng):
            x1, y1 = int(rng.integers(-20, w - 30)), int(rng.integers(-20, h - 30))
            b = np.array([x1, y1, x1 + int(rng.integers(15, 200)), y1 + int(rng.integers(15, 150))], np.int32)
            if k == 0:
                b = np.array([-25, -10, 40, 30], np.int32)           # negative coordinates: NumPy wraps the slice starts
            m = np.zeros(shape, dtype=bool)
            m[b[1]:b[3], b[0]:b[2]] = True
            gts.append(pdq.GroundTruthInstance(m, int(rng.integers(0, 3)), 0, 0, bounding_box=b))
        dets = []
        for k in range(nd):
            x1, y1 = int(rng.integers(-10, w - 40)), int(rng.integers(-10, h - 40))
            b = np.array([x1, y1, x1 + int(rng.integers(20, 250)), y1 + int(rng.integers(20, 150))], np.int32)
            if k == 0:
                b = np.array([-8, -6, w + 12, h + 9], np.int32)          # off every edge
            s = sigma[k % len(sigma)]
            dets.append(pdq.PBoxDetInst(rng.dirichlet(np.ones(3)), b, [_cov(rng, s, s * 0.8), _cov(rng, s * 1.1, s)]))
        out.append((gts, dets))
    return out


def _device_losses(frames, shape, heatmaps=True):
    recs = [pdq.box_frame_from_instances(g, d, shape) for g, d in frames]
    dets = [pdq._det_arrays(r[4]) for r in recs]
    return engine.pdq_frames(shape, [len(r[1]) for r in recs], np.concatenate([r[0] for r in recs]), [len(r[4]) for r in recs],
                             np.concatenate([d[0] for d in dets]), np.concatenate([d[1] for d in dets]), device=0, heatmaps=heatmaps)


def _check_frames(frames, shape, cpu_rtol=1e-5):
    fg, bg, dbg, heat = _device_losses(frames, shape)
    d0 = 0
    excused = 0
    for f, (gts, dets) in enumerate(frames):
        hm = heat[d0:d0 + len(dets)]
        d0 += len(dets)
        for k, d in enumerate(dets):
            excused += _maps_close(hm[k], d.calc_heatmap(shape))
        # the reductions alone: float64 sums of NumPy's float32 per-pixel terms on the device's heatmaps
        f_terms = pdq._log(hm).astype(np.float64)
        b_terms = (pdq._log(1 - hm) * (hm > 0)).astype(np.float64)
        np.testing.assert_allclose(dbg[f], b_terms.sum(axis=(1, 2)), rtol=2e-7, atol=0)
        for g, gt in enumerate(gts):
            b = gt.bounding_box
            keep = np.ones(shape, dtype=bool)
            keep[b[1]:b[3] + 1, b[0]:b[2] + 1] = False
            np.testing.assert_allclose(fg[f][g], f_terms[:, gt.segmentation_mask].sum(axis=1), rtol=2e-7, atol=0)
            np.testing.assert_allclose(bg[f][g], b_terms[:, keep].sum(axis=1), rtol=2e-7, atol=0)
        if gts and dets:
            cf, cb, cdbg, _ = pdq.pair_losses(gts, dets)
            np.testing.assert_allclose(fg[f], cf, rtol=cpu_rtol)
            np.testing.assert_allclose(bg[f], cb, rtol=cpu_rtol, atol=1e-3)
            np.testing.assert_allclose(dbg[f], cdbg, rtol=cpu_rtol, atol=1e-3)
        else:
            assert fg[f].size == 0 and bg[f].size == 0
    assert excused <= 20


def test_full_size_frames_against_numpy_and_cpu():
    rng = np.random.default_rng(2024)
    _check_frames(_frames(rng, (720, 1280), 4, sigma=(1.2, 2.5, 4.0)), (720, 1280))
    _check_frames(_frames(rng, (375, 1300), 3, sigma=(1.5, 3.0)), (375, 1300))


def test_wide_corners_on_a_reduced_canvas():
    rng = np.random.default_rng(7)
    # wide maps are mostly 0 or 1: sums of ~10^4 equal terms, where the CPU path's float32 tensordot itself drifts by ~2e-5
    # (the device's fp64 sums are held to 2e-7 against float64 sums of the same terms above)
    _check_frames(_frames(rng, (90, 120), 3, sigma=(40.0, 130.0, 70.0), n_gt=3, n_det=3), (90, 120), cpu_rtol=1e-4)


def test_bitwise_repeatable_and_batch_independent():
    rng = np.random.default_rng(99)
    shape = (200, 320)
    frames = _frames(rng, shape, 5, sigma=(3.0, 15.0, 40.0))
    a = _device_losses(frames, shape, heatmaps=False)
    b = _device_losses(frames, shape, heatmaps=False)
    for x, y in zip(a[:3], b[:3]):
        for u, v in zip(x, y):
            assert u.tobytes() == v.tobytes()
    for f in range(len(frames)):
        one = _device_losses(frames[f:f + 1], shape, heatmaps=False)
        for k in range(3):
            assert one[k][0].tobytes() == a[k][f].tobytes(), (f, k)


def test_offline_eval_cli_on_device_matches_cpu(tmp_path):
    from test_offline_eval import SHAPE as TREE_SHAPE, _tree
    root, labels, _ = _tree(tmp_path, clutter=3)
    size = ['--image-size', str(TREE_SHAPE[0]), str(TREE_SHAPE[1])]
    cpu = offline_eval.main(['pdq', '--labels', labels, '--predictions', root] + size)
    gpu = offline_eval.main(['pdq', '--labels', labels, '--predictions', root] + size + ['--gpu-device', '0'])
    _same_report(cpu, gpu)
    # KITTI form: label_2 files, a 375 x 1300 canvas, boxes clipped to 1300
    rng = np.random.default_rng(9)
    from bayes_od_rc_amd import box_utils
    from bayes_od_rc_amd.writers import PredictionWriter
    label_dir = tmp_path / 'label_2'
    label_dir.mkdir()
    w = PredictionWriter(str(tmp_path / 'kitti'), 'kitti', 3)
    for f in range(3):
        rows, vuvu, cls5, cls8 = [], [], [], []
        for _ in range(3):
            x1, y1 = int(rng.integers(10, 1200)), int(rng.integers(10, 300))
            bw, bh = int(rng.integers(40, 200)), int(rng.integers(40, 100))
            c = int(rng.integers(0, 2))
            rows.append('%s 0.00 0 -10 %d.00 %d.00 %d.00 %d.00 1 1 1 0 0 0 0' % (('Car', 'Pedestrian')[c], x1, y1, x1 + bw, y1 + bh))
            vuvu.append([y1 + rng.integers(-5, 5), x1 + rng.integers(-5, 5), y1 + bh, x1 + bw])
            p5 = np.full(5, 0.02, np.float32); p5[c] = 0.92
            p8 = np.full(8, 0.01, np.float32); p8[0 if c == 0 else 3] = 0.93
            cls5.append(p5); cls8.append(p8)
        (label_dir / ('%06d.txt' % f)).write_text('\n'.join(rows) + '\n')
        vuvu = np.array(vuvu, np.float32)
        w.write('%06d' % f, vuvu, np.array(cls5), box_utils.vuvu_to_vuhw_np(vuvu), np.tile(np.eye(4, dtype=np.float32)[None] * 0.05, (3, 1, 1)),
                np.array(cls8), np.array(cls8) * 30)
    w.close()
    cpu = offline_eval.main(['pdq', '--dataset', 'kitti', '--labels', str(label_dir), '--predictions', w.root])
    gpu = offline_eval.main(['pdq', '--dataset', 'kitti', '--labels', str(label_dir), '--predictions', w.root, '--gpu-device', '0'])
    _same_report(cpu, gpu)


def _same_report(cpu, gpu):
    assert [cpu[k] for k in ('TP', 'FP', 'FN')] == [gpu[k] for k in ('TP', 'FP', 'FN')]
    assert abs(cpu['score'] - gpu['score']) < 1e-3
    for k in ('avg_spatial_quality', 'avg_label_quality', 'avg_overall_quality'):
        assert abs(cpu[k] - gpu[k]) < 1e-5, k


def test_invalid_covariances_raise():
    gts, dets = _golden_image(0)
    bad = [np.array([[-1.0, 0.0], [0.0, 2.0]]), np.array([[1.0, 3.0], [3.0, 1.0]]), np.array([[np.nan, 0.0], [0.0, 1.0]])]
    for c in bad:
        d = pdq.PBoxDetInst(G["pbox_probs"][0], G["pbox_boxes"][0], [c, np.eye(2)])
        with pytest.raises(ValueError):
            pdq.PDQ(device=0).score([(gts, [d])])
    with pytest.raises(ValueError):
        engine.pdq_corner_heatmaps(SHAPE, [[5.0, 5.0]], [[[1.0, 2.0], [2.0, 1.0]]], device=0)
