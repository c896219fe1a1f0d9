"""Offline evaluation drivers over the prediction tree ``run_inference`` writes (SURVEY.md section 8 row f4;
reference: src/retina_net/offline_eval/bdd/compute_ap.py:55-78, compute_uncertainty_error.py:60-137,
compute_pdq.py:64-160 -- the KITTI twins differ only in how the label files are read).

The reference scripts hard-code their paths and print a table; here the same computations are functions of
(ground-truth records, prediction tree) plus a small CLI:

    python -m bayes_od_rc_amd.offline_eval ap  --labels val.json --predictions <..>/bayes_od_none
    python -m bayes_od_rc_amd.offline_eval mue --labels val.json --predictions <..>/bayes_od_none --entropy gaussian
    python -m bayes_od_rc_amd.offline_eval pdq --labels val.json --predictions <..>/bayes_od_none --image-size 720 1280

    python -m bayes_od_rc_amd.offline_eval ap|pdq --dataset kitti --labels <label_2 dir> --predictions <..>/bayes_od_none

``pdq --gpu-device N`` computes the per-pair losses on GPU N (bod_pdq_frames, pdq_kernels.hip); the rest is the same code.

    python -m bayes_od_rc_amd.offline_eval scores --labels val.json --predictions <..>/bayes_od_none [--gpu-device N] [--parts]

``scores`` reports proper scoring rules and calibration of the predictive distributions (scoring_rules.py: NLL, energy
score, PIT calibration error, the covariance scale that minimises the NLL, classification NLL / Brier / ECE).

    python -m bayes_od_rc_amd.offline_eval shift --labels val.json --predictions clean=<tree> fog3=<tree> [..] [--gpu-device N] [--json]

``shift`` runs the ``scores`` computation on every named tree -- a clean run and runs under ``run_inference --corrupt
NAME:SEVERITY`` -- and prints one table: every scalar ``scores`` metric per name and its difference to the
first name's.

``--predictions`` is the directory holding ``data/ mean/ cov/ cat_param/`` (run_inference.py:90-115); labels are
BDD-format records ``{name, category, bbox: [x1, y1, x2, y2]}`` or, for KITTI, the label_2 text files (converted to the
same records by ``kitti_records``).  Host NumPy like the reference.
"""
import argparse
import json
import os

import numpy as np

from . import evaluation_utils_2d as ev
from . import prob_detection_quality as pdq
from .box_utils import vuhw_to_vuvu_np

BDD_CATEGORIES = ('car', 'truck', 'bus', 'person', 'rider', 'bike', 'motor')


def ap_report(gt_records, prediction_records, iou_threshold=0.5):
    """compute_ap.py:55-77: per-category AP at one IoU threshold, means over the categories that have ground truth
    (AP > 0), and the share of predictions whose category the label set does not contain."""
    mean_ap, aps, cat_list, opt_thr, max_f = ev.evaluate_detection(gt_records, prediction_records, iou_thresholds=[iou_threshold])
    aps_a = np.array(aps)
    seen = aps_a > 0.0
    ood = np.array([0 if p['category'] in cat_list else 1 for p in prediction_records])
    return {'mean_ap': float(np.mean(aps_a[seen])) if seen.any() else 0.0,
            'mean_max_f_score': float(np.mean(np.array(max_f)[seen])) if seen.any() else 0.0,
            'mean_optimal_score_threshold': float(np.mean(np.array(opt_thr)[seen])) if seen.any() else 0.0,
            'out_of_distribution_ratio': float(np.sum(ood) / max(len(prediction_records), 1)),
            'categories': list(cat_list), 'ap': [float(a) for a in aps]}


def _load(tree, sub, frame):
    return np.load(os.path.join(tree, sub, frame) + '.npy')


def entropy_ranked_predictions(tree, frames, category_names=BDD_CATEGORIES + ('bkgrnd',), entropy_method='gaussian',
                               compute_method='Categorical'):
    """compute_uncertainty_error.py:84-128: one record per detection with its class (arg-max of the categorical
    parameters) and the entropy it is ranked by."""
    records = []
    for frame in frames:
        means = _load(tree, 'mean', frame)
        if not means.size:
            continue
        boxes = vuhw_to_vuvu_np(means)
        cats = _load(tree, 'cat_param', frame)
        covs = _load(tree, 'cov', frame)
        names = [category_names[i] for i in np.argmax(cats, axis=1)]
        if entropy_method == 'gaussian':
            ent = [ev.compute_gaussian_entropy_np(c) for c in covs]
        elif entropy_method == 'categorical':
            ent = [ev.compute_categorical_entropy_np(c) for c in cats]
        else:
            raise ValueError('Invalid entropy method: %s' % entropy_method)
        for b, name, e in zip(boxes, names, ent):
            b = b.tolist()
            records.append({'name': frame, 'category': 'All' if compute_method == 'All' else name,
                            'bbox': [b[1], b[0], b[3], b[2]], 'entropy_score': e})
    return records


def uncertainty_error_report(gt_records, tree, frames, category_names=BDD_CATEGORIES + ('bkgrnd',), entropy_method='gaussian',
                             compute_method='Categorical', iou_threshold=0.5):
    """compute_uncertainty_error.py:66-137: minimum uncertainty error per category and its mean."""
    gt = [dict(g) for g in gt_records if g['category'] in category_names]
    if compute_method == 'All':
        for g in gt:
            g['category'] = 'All'
    pred = entropy_ranked_predictions(tree, frames, category_names, entropy_method, compute_method)
    mues, mean_mue, cat_list, _ = ev.evaluate_u_error(gt, pred, iou_thresholds=[iou_threshold])
    return {'mean_mue': float(mean_mue), 'categories': list(cat_list), 'mue': [float(m) for m in mues]}


def read_bdd_frame(frame, gt_records, categories=BDD_CATEGORIES):
    """One frame's (one-hot classes [G, C+1], boxes [G, 4] as x1 y1 x2 y2); a frame without labelled objects yields one
    background-class unit box, as the reference's reader does (demos/demo_utils/bdd_demo_utils.py:4-61, pdq_eval=True):
    it is too small to count but takes part in the assignment."""
    return _bdd_frame_arrays([g for g in gt_records if g['name'] == frame], categories)


def _bdd_frame_arrays(frame_records, categories=BDD_CATEGORIES):
    rows = [g for g in frame_records if g['category'] in categories]
    if not rows:
        onehot = np.zeros((1, len(categories) + 1), np.float32)
        onehot[0, len(categories)] = 1
        return onehot, np.array([[0.0, 0.0, 1.0, 1.0]], np.float32)
    onehot = np.zeros((len(rows), len(categories) + 1), np.float32)
    for k, g in enumerate(rows):
        onehot[k, categories.index(g['category'].lower())] = 1
    return onehot, np.array([g['bbox'] for g in rows], np.float32)


def _records_by_frame(gt_records):
    """{name: that frame's records in file order}: one pass instead of read_bdd_frame's scan per frame."""
    out = {}
    for g in gt_records:
        out.setdefault(g['name'], []).append(g)
    return out


# ---------------------------------------------------------------------------------------------------------------
# KITTI twins (offline_eval/kitti/compute_ap.py:40-80, compute_pdq.py:59-125): labels are label_2 text files, the
# box predictions are the per-frame text files run_inference writes into data/ (validation_utils.py:217-272).
# ---------------------------------------------------------------------------------------------------------------
_KITTI_ONEHOT = {'car': [1, 0, 0, 0], 'pedestrian': [0, 1, 0, 0], 'person_sitting': [0, 1, 0, 0], 'cyclist': [0, 0, 1, 0]}


def _kitti_rows(path, ncols):
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                           # (an empty prediction file)
        rows = np.loadtxt(path, delimiter=' ', dtype=str, usecols=np.arange(ncols), ndmin=2)
    return rows


def read_kitti_labels(label_path, difficulty='hard', categories=('car', 'pedestrian', 'cyclist')):
    """(one-hot [G, 4], boxes [G, 4] as v1 u1 v2 u2) of the objects passing the difficulty filter
    (demos/demo_utils/kitti_demo_utils.py:8-68); empty arrays when nothing passes."""
    from .datasets import KITTI_DIFF_DICTS, kitti_labels_to_boxes_2d
    rows = _kitti_rows(label_path, 15)
    d = KITTI_DIFF_DICTS[difficulty.lower()]
    if rows.size:
        heights = rows[:, 7].astype(np.float32) - rows[:, 5].astype(np.float32)
        keep = (np.asarray([c.lower() in categories for c in rows[:, 0]], dtype=bool) & (heights >= d['min_height'])
                & (rows[:, 1].astype(np.float64) <= d['max_truncation']) & (rows[:, 2].astype(np.float64) <= d['max_occlusion']))
        rows = rows[keep]
    if not rows.size:
        return np.zeros((0, 4), np.float32), np.zeros((0, 4), np.float32)
    onehot = [_KITTI_ONEHOT[c.lower()] for c in rows[:, 0] if c.lower() in _KITTI_ONEHOT]
    return np.array(onehot, np.float32), kitti_labels_to_boxes_2d(rows).astype(np.float32)


def read_kitti_predictions(prediction_path, categories=('car', 'pedestrian', 'cyclist', 'dontcare')):
    """(one-hot [D, 4], boxes [D, 4] as v1 u1 v2 u2, scores [D]) of one frame's prediction file (:71-127)."""
    from .datasets import kitti_labels_to_boxes_2d
    rows = _kitti_rows(prediction_path, 16)
    if rows.size:
        rows = rows[np.asarray([c.lower() in categories for c in rows[:, 0]], dtype=bool)]
    if not rows.size:
        return np.zeros((0, 4), np.float32), np.zeros((0, 4), np.float32), np.zeros((0,), np.float32)
    onehot = [_KITTI_ONEHOT[c.lower()] for c in rows[:, 0] if c.lower() in _KITTI_ONEHOT]
    return np.array(onehot, np.float32), kitti_labels_to_boxes_2d(rows).astype(np.float32), rows[:, 15].astype(np.float32)


def kitti_records(label_dir, tree, difficulty='all', categories=('car', 'pedestrian')):
    """(ground-truth records, prediction records) in the BDD record form, one 'name' per frame index, frames where
    either side is empty skipped -- exactly what kitti/compute_ap.py:40-72 hands to evaluate_detection."""
    gt, pred = [], []
    frames = sorted(os.listdir(os.path.join(tree, 'data')))
    for idx, frame in enumerate(frames):
        fid = int(frame[0:6])
        g_cls, g_box = read_kitti_labels(os.path.join(label_dir, '%06d.txt' % fid), difficulty, categories)
        p_cls, p_box, p_score = read_kitti_predictions(os.path.join(tree, 'data', '%06d.txt' % fid), categories)
        if not (g_box.size and p_box.size):
            continue
        for c, b in zip(g_cls, g_box):
            gt.append({'name': str(idx), 'category': categories[int(np.argmax(c))], 'bbox': [float(b[1]), float(b[0]), float(b[3]), float(b[2])], 'score': 1})
        for c, b, sc in zip(p_cls, p_box, p_score):
            pred.append({'name': str(idx), 'category': categories[int(np.argmax(c))], 'bbox': [float(b[1]), float(b[0]), float(b[3]), float(b[2])],
                         'score': float(sc)})
    return gt, pred


def kitti_pdq_report(label_dir, tree, difficulty='all', categories=('car', 'pedestrian'), img_shape=(375, 1300), device=None):
    """kitti/compute_pdq.py:59-135: every frame of the tree in ONE evaluation.  ``device`` = a GPU index: the losses come
    from bod_pdq_frames (pdq_kernels.hip), the rest of the evaluation is the same host code."""
    matches = []
    convert = pdq.frame_instances if device is None else pdq.frame_boxes
    for frame in sorted(os.listdir(os.path.join(tree, 'mean'))):
        fid = int(frame[0:6])
        g_cls, g_box = read_kitti_labels(os.path.join(label_dir, '%06d.txt' % fid), difficulty, categories)
        name = '%06d' % fid
        matches.append(convert(g_cls, g_box, _load(tree, 'mean', name), _load(tree, 'cov', name), _load(tree, 'cat_param', name),
                               tuple(img_shape), score_threshold=0.5, class_columns=(0, 3), gt_boxes_vuvu=True, clip_max=1300))
    if device is None:
        return pdq.evaluate(matches)
    return pdq.evaluate_boxes(matches, tuple(img_shape), device)


def pdq_report(gt_records, tree, frames, img_shape, categories=BDD_CATEGORIES, chunk=1000, score_threshold=0.5445, device=None):
    """compute_pdq.py:64-160: PDQ per chunk of 1000 frames, chunk scores averaged, counts summed.  Frames whose
    prediction files are empty are skipped (as the reference does).  ``device`` = a GPU index: each chunk's losses come
    from bod_pdq_frames (pdq_kernels.hip), without a mask per object; the label records are grouped by frame once."""
    rows = []
    by_frame = _records_by_frame(gt_records) if device is not None else None
    for lo in range(0, len(frames), chunk):
        matches = []
        for frame in frames[lo:lo + chunk]:
            covs = _load(tree, 'cov', frame)
            if not covs.size:
                continue
            if device is None:
                onehot, boxes = read_bdd_frame(frame, gt_records, categories)
                matches.append(pdq.frame_instances(onehot, boxes, _load(tree, 'mean', frame), covs, _load(tree, 'cat_param', frame),
                                                   tuple(img_shape), score_threshold=score_threshold))
            else:
                onehot, boxes = _bdd_frame_arrays(by_frame.get(frame, []), categories)
                matches.append(pdq.frame_boxes(onehot, boxes, _load(tree, 'mean', frame), covs, _load(tree, 'cat_param', frame),
                                               tuple(img_shape), score_threshold=score_threshold))
        if matches:
            rows.append(pdq.evaluate(matches) if device is None else pdq.evaluate_boxes(matches, tuple(img_shape), device))
    if not rows:
        return {'score': 0.0, 'TP': 0, 'FP': 0, 'FN': 0, 'avg_spatial_quality': 0.0, 'avg_label_quality': 0.0, 'avg_overall_quality': 0.0}
    out = {k: float(np.mean([r[k] for r in rows])) for k in ('score', 'avg_spatial_quality', 'avg_label_quality', 'avg_overall_quality')}
    out.update({k: int(sum(r[k] for r in rows)) for k in ('TP', 'FP', 'FN')})
    return out


def _scalar_metrics(report, prefix=''):
    """The report's numbers as a flat {name: value} (nested dicts joined with '.'; lists such as histograms left out)."""
    flat = {}
    for k, v in report.items():
        if isinstance(v, dict):
            flat.update(_scalar_metrics(v, prefix + k + '.'))
        elif v is None or (isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool)):
            flat[prefix + k] = None if v is None else float(v)
    return flat


def shift_report(gt_records, trees, **score_kw):
    """The ``scores`` report of every (name, tree) of ``trees`` -- the same labels, say a clean run and runs under
    ``run_inference --corrupt`` -- and every scalar metric's difference to the first name's.  Returns {'names', 'reports': {name:
    scores report}, 'metrics': {name: {metric: value}}, 'delta': {name: {metric: value - first name's, None where either is}}}."""
    from . import scoring_rules                       # (imports this module)
    trees = list(trees)
    if not trees:
        raise ValueError('shift needs at least one NAME=TREE')
    names = [n for n, _ in trees]
    if len(set(names)) != len(names):
        raise ValueError('shift: the names must differ: %s' % ', '.join(names))
    reports, metrics = {}, {}
    for name, tree in trees:
        frames = sorted(f[:-4] for f in os.listdir(os.path.join(tree, 'mean')) if f.endswith('.npy'))
        reports[name] = scoring_rules.scores_report(gt_records, tree, frames, **score_kw)
        metrics[name] = _scalar_metrics(reports[name])
    base = metrics[names[0]]
    delta = {n: {k: (None if v is None or base.get(k) is None else v - base[k]) for k, v in metrics[n].items()} for n in names}
    return {'names': names, 'reports': reports, 'metrics': metrics, 'delta': delta}


def format_shift_table(out):
    """One row per name and metric column pair: the value, and its difference to the first name's in brackets."""
    names = out['names']
    keys = [k for k in out['metrics'][names[0]]]
    width = max(len(k) for k in keys + ['metric'])
    lines = ['%-*s  %s' % (width, 'metric', '  '.join('%24s' % n[:24] for n in names))]

    def cell(name, k):
        v, d = out['metrics'][name].get(k), out['delta'][name].get(k)
        if v is None:
            return '%24s' % '-'
        return '%24s' % ('%.6g' % v if name == names[0] or d is None else '%.6g (%+.4g)' % (v, d))
    for k in keys:
        lines.append('%-*s  %s' % (width, k, '  '.join(cell(n, k) for n in names)))
    return '\n'.join(lines)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('metric', choices=('ap', 'mue', 'pdq', 'scores', 'shift'))
    ap.add_argument('--labels', required=True, help='BDD-format ground-truth json, or (with --dataset kitti) the label_2 directory')
    ap.add_argument('--dataset', default='bdd', choices=('bdd', 'kitti'))
    ap.add_argument('--difficulty', default='all', choices=('easy', 'moderate', 'hard', 'all'))
    ap.add_argument('--predictions', required=True, nargs='+', metavar='TREE', help='directory with data/ mean/ cov/ cat_param/; '
                    'shift: NAME=TREE [NAME=TREE ...], the first one being the reference (the clean run)')
    ap.add_argument('--json', action='store_true', help='shift: print the whole result as JSON after the table')
    ap.add_argument('--entropy', default='gaussian', choices=('gaussian', 'categorical'))
    ap.add_argument('--compute-method', default='Categorical', choices=('Categorical', 'All'))
    ap.add_argument('--image-size', type=int, nargs=2, default=(720, 1280), metavar=('H', 'W'))
    ap.add_argument('--gpu-device', type=int, default=None, metavar='N',
                    help='pdq: compute the losses on GPU N (pdq_kernels.hip); scores: score the pairs on GPU N (score_kernels.hip)')
    ap.add_argument('--samples', type=int, default=1000, metavar='M', help='scores: Gaussian samples per pair of the energy score')
    ap.add_argument('--seed', type=int, default=0, help='scores: seed of the energy score\'s samples')
    ap.add_argument('--cov-scale', type=float, default=1.0, metavar='X', help='scores: factor on every covariance before scoring')
    ap.add_argument('--score-threshold', type=float, default=0.5445, metavar='T', help='scores: lowest best-class score of a detection')
    ap.add_argument('--parts', action='store_true', help='scores: also score the epistemic / aleatoric covariance parts')
    args = ap.parse_args(argv)
    if args.metric == 'shift':
        if args.dataset == 'kitti':
            raise SystemExit('shift --dataset kitti: convert the labels to records with kitti_records() and call shift_report()')
        trees = []
        for item in args.predictions:
            name, sep, tree = item.partition('=')
            if not sep or not name or not tree:
                ap.error('shift: --predictions takes NAME=TREE, got %r' % item)
            trees.append((name, tree))
        with open(args.labels) as fp:
            gt = json.load(fp)
        try:
            out = shift_report(gt, trees, score_threshold=args.score_threshold, cov_scale=args.cov_scale, num_samples=args.samples,
                               seed=args.seed, device=args.gpu_device, parts=args.parts)
        except ValueError as e:
            ap.error(str(e))
        print(format_shift_table(out))
        if args.json:
            print(json.dumps(out, indent=1))
        return out
    if len(args.predictions) != 1:
        ap.error('%s takes one --predictions directory' % args.metric)
    args.predictions = args.predictions[0]
    if args.dataset == 'kitti':
        if args.metric == 'ap':
            out = ap_report(*kitti_records(args.labels, args.predictions, args.difficulty))
        elif args.metric == 'pdq':
            out = kitti_pdq_report(args.labels, args.predictions, args.difficulty, device=args.gpu_device)
        elif args.metric == 'scores':
            raise SystemExit('scores --dataset kitti: convert the labels to records with kitti_records() and call scoring_rules.scores_report()')
        else:
            raise SystemExit('mue --dataset kitti: convert the labels to records with kitti_records() and call uncertainty_error_report()')
        print(json.dumps(out, indent=1))
        return out
    with open(args.labels) as fp:
        gt = json.load(fp)
    if args.metric == 'ap':
        with open(os.path.join(args.predictions, 'data', 'predictions.json')) as fp:
            out = ap_report(gt, json.load(fp))
    else:
        frames = sorted(f[:-4] for f in os.listdir(os.path.join(args.predictions, 'mean')) if f.endswith('.npy'))
        if args.metric == 'mue':
            out = uncertainty_error_report(gt, args.predictions, frames, entropy_method=args.entropy, compute_method=args.compute_method)
        elif args.metric == 'scores':
            from . import scoring_rules                   # (imports this module)
            out = scoring_rules.scores_report(gt, args.predictions, frames, score_threshold=args.score_threshold, cov_scale=args.cov_scale,
                                              num_samples=args.samples, seed=args.seed, device=args.gpu_device, parts=args.parts)
        else:
            out = pdq_report(gt, args.predictions, frames, args.image_size, device=args.gpu_device)
    print(json.dumps(out, indent=1))
    return out


if __name__ == '__main__':
    main()
