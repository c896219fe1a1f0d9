#!/usr/bin/env python3
"""PNG frames decoded inside the library against PIL on the Python thread: 64 KITTI-sized frames of 375x1242 RGB (a smooth
gradient plus noise, written by PIL, kept in memory as bytes) into a KITTI handle whose network input is 384x1248, 16 frames per upload.
Host clock around the whole step of 64 frames, copies and synchronisation included; three routes, alternated, median of three:
  (a) the parent route: PIL decode in the Python loop, then upload_frames_u8_ragged
  (b) upload_frames_png, threads=1
  (c) upload_frames_png, threads=16
and, for the two acceptance comparisons of DESIGN 9.15 (bod_bench_png_decode on one 16-frame batch):
  the host half of an upload alone, on 1 and on 16 of the library's worker threads, by the host clock,
  png_unfilter_kernel alone, by events around each launch,
  the infer rate of the same handle (384x1248, N = 30, batch 16; bod_infer_async + bod_collect) on the frames the last upload left.
usage: bench_png.py   (records go to profiles/png_upload_ab.txt)"""
import io
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
from PIL import Image
from bayes_od_rc_amd import constants, synthetic
from bayes_od_rc_amd.anchor_generator import FpnAnchorGenerator
from bayes_od_rc_amd.engine import Engine, bench_png_decode, decode_png_rgb, make_config, png_info

import torch
assert torch.cuda.is_available()          # (get_images goes through torch: it initialises its runtime before the library's first HIP call)

H, W, NET, FRAMES, B, N = 375, 1242, (384, 1248), 64, 16, 30
rng = np.random.default_rng(0)
yy, xx = np.mgrid[0:H, 0:W]
files, arrays = [], []
for i in range(FRAMES):
    a = np.stack([255.0 * xx / (W - 1), 255.0 * yy / (H - 1), 255.0 - 127.0 * (xx + yy) / (W + H - 2)], axis=2)
    a = np.clip(a + rng.normal(0.0, 12.0, a.shape), 0, 255).astype(np.uint8)
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, "PNG")
    files.append(buf.getvalue())
    arrays.append(a)
file_bytes = sum(len(f) for f in files)
info = png_info(files[0])
print("%d frames of %dx%d RGB: %d file bytes (%.0f KB per frame), %d filtered bytes per frame; batch %d per upload"
      % (FRAMES, H, W, file_bytes, file_bytes / FRAMES / 1e3, info["raw_bytes"], B), flush=True)

# the decoder's two halves apart, on the last batch (bod_bench_png_decode): the host half as an upload runs it -- headers, layout,
# inflate into pinned staging on the library's own worker threads -- and png_unfilter_kernel alone by events
batch = files[FRAMES - B:]
assert all(np.array_equal(g, a) for g, a in zip(decode_png_rgb(batch), arrays[FRAMES - B:]))
host_1, _ = bench_png_decode(batch, threads=1, iters=4)
host_16, kernel_ms = bench_png_decode(batch, threads=16, iters=6)
host_1, host_16 = host_1[1:], host_16[1:]          # (the first iteration allocates the pinned staging)
print("host half, one thread: %s ms per batch of %d, median %.2f ms per frame (%.1f MB/s of file bytes)"
      % (", ".join("%.1f" % t for t in host_1), B, statistics.median(host_1) / B, file_bytes / FRAMES * B / statistics.median(host_1) / 1e3), flush=True)
print("host half, 16 threads: %s ms per batch of %d, median %.2f ms" % (", ".join("%.2f" % t for t in host_16), B, statistics.median(host_16)), flush=True)
t0 = time.perf_counter()
for f in files:
    np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))
print("PIL decode, one thread: %.2f ms per frame" % ((time.perf_counter() - t0) / FRAMES * 1e3), flush=True)
print("png_unfilter_kernel, %d frames of %dx%d: %s ms, median %.3f ms"
      % (B, H, W, ", ".join("%.3f" % t for t in kernel_ms), statistics.median(kernel_ms)), flush=True)

eng = Engine(make_config(NET, batch=B, mc_samples=N, dataset_name="kitti", orig_size=(H, W)))
eng.load_weights(synthetic.make_weights())
eng.set_anchors(FpnAnchorGenerator({"layers": [3, 4, 5, 6, 7], "aspect_ratios": [[1.0, 1.0], [1.0, 2.0], [2.0, 1.0]],
                                    "scales": [1.0, 1.26, 1.59]}).generate_all((NET[0], NET[1], 3)))
MEANS = constants.MEANS_DICT["Kitti"]


def pil_route():
    for first in range(0, FRAMES, B):
        frames = [np.asarray(Image.open(io.BytesIO(f)).convert("RGB")) for f in files[first:first + B]]
        eng.upload_frames_u8_ragged(frames, MEANS, aspect_resize=True)


def png_route(threads):
    for first in range(0, FRAMES, B):
        eng.upload_frames_png(files[first:first + B], MEANS, aspect_resize=True, threads=threads)


routes = [("(a) PIL + upload_frames_u8_ragged", pil_route), ("(b) upload_frames_png threads=1", lambda: png_route(1)),
          ("(c) upload_frames_png threads=16", lambda: png_route(16))]
# same bytes in the image buffer, whichever route filled it
pil_route()
ref = eng.get_images()[-1].copy()
png_route(16)
assert np.array_equal(eng.get_images()[-1], ref)
times = {name: [] for name, _ in routes}
for rep in range(3):
    for name, fn in routes:
        t0 = time.perf_counter()
        fn()
        times[name].append(time.perf_counter() - t0)
rates = {}
for name, _ in routes:
    t = statistics.median(times[name])
    rates[name[:3]] = FRAMES / t
    print("%-36s median of 3: %.1f ms per 64 frames, %.0f frames/s   (runs: %s)"
          % (name, t * 1e3, FRAMES / t, ", ".join("%.1f" % (x * 1e3) for x in times[name])), flush=True)

# the forward the uploads feed: a whole pass on the uploaded batch, its detection records collected (one warm-up, then three)
eng.collect(eng.infer_async(None, seed=1, first_image_id=0))
infer = []
for rep in range(3):
    t0 = time.perf_counter()
    eng.collect(eng.infer_async(None, seed=2 + rep, first_image_id=0))
    infer.append(time.perf_counter() - t0)
infer_rate = B / statistics.median(infer)
print("infer, %dx%d, N = %d, batch %d: median of 3 %.1f ms per batch, %.0f frames/s   (runs: %s)"
      % (NET[0], NET[1], N, B, statistics.median(infer) * 1e3, infer_rate, ", ".join("%.1f" % (x * 1e3) for x in infer)), flush=True)
eng.close()

k_ms, h_ms = statistics.median(kernel_ms), statistics.median(host_16)
print("acceptance 1: route (c) %.0f frames/s %s the infer rate %.0f frames/s: %s"
      % (rates["(c)"], "exceeds" if rates["(c)"] > infer_rate else "is below", infer_rate, "MET" if rates["(c)"] > infer_rate else "NOT MET"))
print("acceptance 2: unfilter kernel %.3f ms per batch of %d %s the 16-thread host inflate %.2f ms of the same batch: %s"
      % (k_ms, B, "is below" if k_ms < h_ms else "exceeds", h_ms, "MET" if k_ms < h_ms else "NOT MET"))
print("(b) against (a): %.2fx" % (rates["(b)"] / rates["(a)"]))
