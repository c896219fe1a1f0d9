#!/usr/bin/env python3
"""JPEG frames decoded inside the library against PIL on the Python thread: 64 frames of 720x1280 (a smooth gradient plus
noise, written by PIL at quality 90, 4:2:0, kept in memory as bytes) into a handle whose network input is the same size, 16 frames per
upload.  Host clock around the whole step of 64 frames, copies and synchronisation included; three routes, alternated, median of three:
  (a) the parent route: PIL decode in the Python loop, then upload_frames_u8_ragged
  (b) upload_frames_jpeg, threads=1
  (c) upload_frames_jpeg, threads=16
and the host's entropy-decode rate of one thread in MB/s of file bytes.  The two kernels alone: tests/tools/jpeg_kernel_time.hip.
usage: bench_jpeg.py   (run it three times; records go to profiles/jpeg_upload_ab.txt)"""
import ctypes as C
import io
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
from PIL import Image
from bayes_od_rc_amd import _lib
from bayes_od_rc_amd.engine import Engine, make_config, jpeg_info

import torch
assert torch.cuda.is_available()          # (get_images goes through torch: it initialises its runtime before the library's first HIP call)

H, W, FRAMES, B = 720, 1280, 64, 16
rng = np.random.default_rng(0)
yy, xx = np.mgrid[0:H, 0:W]
files = []
for i in range(FRAMES):
    a = np.stack([255.0 * xx / (W - 1), 255.0 * yy / (H - 1), 255.0 - 127.0 * (xx + yy) / (W + H - 2)], axis=2)
    a = np.clip(a + rng.normal(0.0, 12.0, a.shape), 0, 255).astype(np.uint8)
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, "JPEG", quality=90, subsampling="4:2:0")
    files.append(buf.getvalue())
file_bytes = sum(len(f) for f in files)
info = jpeg_info(files[0])
print("%d frames of %dx%d, quality 90, 4:2:0: %d file bytes (%.0f KB per frame), %d coefficients per frame; batch %d per upload"
      % (FRAMES, H, W, file_bytes, file_bytes / FRAMES / 1e3, info["coef_count"], B), flush=True)

# the host's entropy decoder alone, one thread
lib = _lib.load()
coefs = np.empty(info["coef_count"], np.int16)
quant = np.zeros((3, 64), np.uint16)
cp, qp = coefs.ctypes.data_as(C.POINTER(C.c_int16)), quant.ctypes.data_as(C.POINTER(C.c_uint16))
for rep in range(3):
    t0 = time.perf_counter()
    for f in files:
        assert lib.bod_jpeg_entropy_decode(f, len(f), cp, coefs.size, qp) == 0
    t = time.perf_counter() - t0
    print("rep %d  host entropy decode, one thread: %.2f ms per frame, %.1f MB/s of file bytes" % (rep, t / FRAMES * 1e3, file_bytes / t / 1e6), flush=True)

eng = Engine(make_config((H, W), batch=B, mc_samples=1))


def pil_route():
    for first in range(0, FRAMES, B):
        frames = [np.asarray(Image.open(io.BytesIO(f)).convert("RGB")) for f in files[first:first + B]]
        eng.upload_frames_u8_ragged(frames, aspect_resize=False)


def jpeg_route(threads):
    for first in range(0, FRAMES, B):
        eng.upload_frames_jpeg(files[first:first + B], aspect_resize=False, threads=threads)


routes = [("(a) PIL + upload_frames_u8_ragged", pil_route), ("(b) upload_frames_jpeg threads=1", lambda: jpeg_route(1)),
          ("(c) upload_frames_jpeg threads=16", lambda: jpeg_route(16))]
# same bytes in the image buffer, whichever route filled it
pil_route()
ref = eng.get_images()[-1].copy()
jpeg_route(16)
assert np.array_equal(eng.get_images()[-1], ref)
times = {name: [] for name, _ in routes}
for rep in range(3):
    for name, fn in routes:
        t0 = time.perf_counter()
        fn()
        times[name].append(time.perf_counter() - t0)
for name, _ in routes:
    t = statistics.median(times[name])
    print("%-36s median of 3: %.1f ms per 64 frames, %.0f frames/s   (runs: %s)"
          % (name, t * 1e3, FRAMES / t, ", ".join("%.1f" % (x * 1e3) for x in times[name])), flush=True)
eng.close()
