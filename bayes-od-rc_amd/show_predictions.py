"""Overlays of a prediction tree, drawn on the GPU: the counterpart of the reference's show_predictions and
show_uncertainty_2d_corners demos for BDD and KITTI.

    python -m bayes_od_rc_amd.show_predictions --predictions <tree> --images <dir> --out <dir> [--labels val.json | --kitti_labels <dir>]
        [--view overlay|heat|both] [--min_score S] [--cov_scale X] [--cov_dir cov] [--line_width t] [--frames N] [--batch B]
        [--categories car truck ..] [--gpu-device 0]

``<tree>`` is what run_inference writes (mean/ cov/ cat_param/, one .npy per frame); a frame's image is ``<images>/<frame>.*``.
Every batch of frames -- of mixed sizes -- is ONE ``render.render_frames`` call per view; the result is written with PIL as
``<out>/<frame>_overlay.png`` and / or ``<out>/<frame>_heat.png``.  ``--cov_dir cov_epistemic`` (etc.) shows one part of a
--covariance_parts tree.  Ground truth (green): a BDD label json (``name`` / ``labels[].box2d``, or the flat records of
predictions.json with ``bbox``) or a directory of KITTI label files."""
import argparse
import json
import os
import sys

import numpy as np

from . import render

BDD_CATEGORIES = ('car', 'truck', 'bus', 'person', 'rider', 'bike', 'motor')
IMAGE_EXTENSIONS = ('.jpg', '.jpeg', '.png', '.bmp')


def find_image(images_dir, frame):
    for ext in IMAGE_EXTENSIONS:
        for e in (ext, ext.upper()):
            path = os.path.join(images_dir, frame + e)
            if os.path.exists(path):
                return path
    raise ValueError("no image for frame %r in %s" % (frame, images_dir))


def read_bdd_boxes(path):
    """frame -> int32 [G,4] x0 y0 x1 y1 from a BDD label file."""
    out = {}
    for rec in json.load(open(path)):
        name = os.path.splitext(rec['name'])[0]
        rows = [rec] if 'bbox' in rec else [l for l in rec.get('labels', []) if 'box2d' in l]
        for r in rows:
            b = r['bbox'] if 'bbox' in r else [r['box2d'][k] for k in ('x1', 'y1', 'x2', 'y2')]
            out.setdefault(name, []).append([int(v) for v in b])
    return {k: np.asarray(v, np.int32).reshape(-1, 4) for k, v in out.items()}


def read_kitti_boxes(labels_dir, frame):
    """int32 [G,4] x0 y0 x1 y1 of one KITTI label file (columns 4..7: left top right bottom); DontCare rows are left out."""
    path = os.path.join(labels_dir, frame + '.txt')
    rows = []
    if os.path.exists(path):
        for line in open(path):
            f = line.split()
            if len(f) >= 8 and f[0] != 'DontCare':
                rows.append([int(float(v)) for v in f[4:8]])
    return np.asarray(rows, np.int32).reshape(-1, 4)


def tree_frames(tree):
    return sorted(os.path.splitext(f)[0] for f in os.listdir(os.path.join(tree, 'mean')) if f.endswith('.npy'))


def render_tree_frames(tree, names, images, views, out_dir, gt=None, device=0, **kw):
    """Renders frames `names` of `tree` onto `images` (uint8 [h,w,3] each) in one call per view and writes the PNGs; returns the paths.
    kw: min_score, cov_scale, categories, cov_dir, line_width."""
    from PIL import Image
    line_width = kw.pop('line_width', 2)
    dets = [render.detections_from_tree(tree, n, **kw) for n in names]
    paths = []
    os.makedirs(out_dir, exist_ok=True)
    for view in views:
        for n, img in zip(names, render.render_frames(images, dets, view=view, line_width=line_width, gt_boxes=gt, device=device)):
            paths.append(os.path.join(out_dir, '%s_%s.png' % (n, view)))
            Image.fromarray(img).save(paths[-1])
    return paths


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--predictions', required=True)
    ap.add_argument('--images', required=True)
    ap.add_argument('--out', required=True)
    ap.add_argument('--labels', default=None, help='BDD label json')
    ap.add_argument('--kitti_labels', default=None, help='directory of KITTI label files')
    ap.add_argument('--view', choices=('overlay', 'heat', 'both'), default='overlay')
    ap.add_argument('--min_score', type=float, default=0.5)
    ap.add_argument('--cov_scale', type=float, default=1.0)
    ap.add_argument('--cov_dir', default='cov')
    ap.add_argument('--line_width', type=int, default=2)
    ap.add_argument('--frames', type=int, default=None, help='only the first N frames of the tree')
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--categories', nargs='+', default=list(BDD_CATEGORIES))
    ap.add_argument('--gpu-device', '--gpu_device', dest='gpu_device', type=int, default=0)
    args = ap.parse_args(argv)
    from PIL import Image
    names = tree_frames(args.predictions)[:args.frames]
    views = ('overlay', 'heat') if args.view == 'both' else (args.view,)
    bdd = read_bdd_boxes(args.labels) if args.labels else None
    written = 0
    for lo in range(0, len(names), max(1, args.batch)):
        chunk = names[lo:lo + max(1, args.batch)]
        images = [np.asarray(Image.open(find_image(args.images, n)).convert('RGB')) for n in chunk]
        gt = None
        if bdd is not None:
            gt = [bdd.get(n, np.zeros((0, 4), np.int32)) for n in chunk]
        elif args.kitti_labels:
            gt = [read_kitti_boxes(args.kitti_labels, n) for n in chunk]
        written += len(render_tree_frames(args.predictions, chunk, images, views, args.out, gt=gt, device=args.gpu_device,
                                          min_score=args.min_score, cov_scale=args.cov_scale, categories=args.categories,
                                          cov_dir=args.cov_dir, line_width=args.line_width))
        sys.stdout.write('\r%d / %d' % (lo + len(chunk), len(names)))
    print("\n%d files in %s" % (written, args.out))
    return 0


if __name__ == '__main__':
    sys.exit(main())
