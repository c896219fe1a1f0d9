#!/usr/bin/env python3
"""Training-time augmentation at the yaml's KITTI training shape -- network 512x1696, minibatch 3, three KITTI source
sizes in one batch: the augmented upload against the ragged upload of the same frames (same bytes moved), and one training step
from boxes with and without augmentation.  usage: bench_augment.py"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")           # as run_training sets it
import numpy as np
from bayes_od_rc_amd import constants, synthetic
from bayes_od_rc_amd.anchor_generator import FpnAnchorGenerator
from bayes_od_rc_amd.engine import Engine, make_config, draw_augmentation, augment_boxes

H, W, B = 512, 1696, 3
ACFG = {'layers': [3, 4, 5, 6, 7], 'aspect_ratios': [[1, 1], [1, 2], [2, 1]], 'scales': [1.0, 1.26, 1.59], 'min_positive_iou': 0.5, 'max_negative_iou': 0.4}
sizes = [(370, 1224), (375, 1242), (376, 1241)]
rng = np.random.default_rng(0)
frames = [rng.integers(0, 256, size=hw + (3,), dtype=np.uint8) for hw in sizes]
means = constants.MEANS_DICT['Kitti']
src_bytes = sum(f.size for f in frames)
dst_bytes = B * H * W * 3 * 4
print("frames", sizes, "network %dx%d batch %d: %d source bytes over PCIe, %d bytes written by the kernel" % (H, W, B, src_bytes, dst_bytes), flush=True)

eng = Engine(make_config((H, W), batch=B, mc_samples=1, training=True, num_classes=4))
eng.load_weights(synthetic.make_weights(4, 9))
anchors = FpnAnchorGenerator(ACFG).generate_all((H, W, 3)).astype(np.float32)
eng.set_anchors(anchors)
ident = draw_augmentation({"flip_probability": 0.0, "scale_range": [1.0, 1.0], "random_placement": False, "gain_range": [1.0, 1.0], "bias_range": [0.0, 0.0]}, 0, range(B))
drawn = draw_augmentation(None, 1, range(B))

def time_upload(fn, n=40):
    fn(); fn()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()                                              # synchronous: returns after the kernel has finished
    return (time.perf_counter() - t0) / n

print("(b) upload: host clock around the synchronous call (pack on the host + H2D copy + kernel + synchronise), 40 calls each, alternated")
for rep in range(3):
    tr = time_upload(lambda: eng.upload_frames_u8_ragged(frames, means, aspect_resize=True))
    ti = time_upload(lambda: eng.upload_frames_u8_augmented(frames, ident, means, aspect_resize=True))
    ta = time_upload(lambda: eng.upload_frames_u8_augmented(frames, drawn, means, aspect_resize=True))
    for name, t in (("ragged", tr), ("augmented, identity records", ti), ("augmented, drawn records", ta)):
        print("rep %d  %-30s %.3f ms/call  %.2f GB/s source  %.2f GB/s source+written" % (rep, name, t * 1e3, src_bytes / t / 1e9, (src_bytes + dst_bytes) / t / 1e9), flush=True)

# (c) one training step from boxes, with and without augmentation (ground truth: 4 boxes per frame in source pixels)
src_boxes = [np.asarray([[100, 200, 250, 500], [150, 600, 300, 900], [50, 50, 120, 160], [200, 1000, 340, 1200]], np.float32)] * B
classes = [np.eye(4, dtype=np.float32)[[0, 1, 2, 0]]] * B
net_boxes = [(b / np.asarray([h, w, h, w], np.float32)) * np.asarray([H, W, H, W], np.float32) for b, (h, w) in zip(src_boxes, sizes)]
step = [0]

def plain():
    eng.upload_frames_u8_ragged(frames, means, aspect_resize=True)
    out = eng.train_step_boxes(None, net_boxes, classes, 0.5, 0.4, seed=1, first_image_id=step[0] * B)
    step[0] += 1
    return out

def augmented():
    first = step[0] * B
    aug = draw_augmentation(None, 1, range(first, first + B))
    eng.upload_frames_u8_augmented(frames, aug, means, aspect_resize=True)
    bx, cl = augment_boxes(sizes, (H, W), aug, src_boxes, classes, aspect_resize=True, min_visible=0.25)
    out = eng.train_step_boxes(None, bx, cl, 0.5, 0.4, seed=1, first_image_id=first)
    step[0] += 1
    return out

print("(c) training step ResNet-50 %dx%d batch %d from boxes: upload + step, host clock, 10 steps each after 3 warm-up steps, alternated" % (H, W, B))
for fn in (plain, augmented):
    for _ in range(3):
        fn()
for rep in range(3):
    for name, fn in (("ragged upload + step", plain), ("draw + augmented upload + boxes + step", augmented)):
        t0 = time.perf_counter()
        for _ in range(10):
            out = fn()
        dt = (time.perf_counter() - t0) / 10
        print("rep %d  %-40s %.2f ms/step  %.1f frames/s  loss %.3f" % (rep, name, dt * 1e3, B / dt, out["total_loss"]), flush=True)
t0 = time.perf_counter()
for i in range(200):
    aug = draw_augmentation(None, 1, range(i * B, i * B + B))
    augment_boxes(sizes, (H, W), aug, src_boxes, classes, aspect_resize=True, min_visible=0.25)
print("host share of the augmented step: draw_augmentation + augment_boxes %.3f ms/step" % ((time.perf_counter() - t0) / 200 * 1e3))
eng.close()
