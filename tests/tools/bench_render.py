"""Measures the rendering stage.  Not a test: it asserts no time.

    python tests/tools/bench_render.py [--frames 16] [--heat-frames 4] [--window 2.0] [--out FILE]

Per frame size (720x1280, 375x1242), detections per frame (10, 100) and view:
  * device ms of bod_render_frames_u8's kernels by events (BOD_RENDER_TRACE=1: binning and painting apart for the overlay; for the
    heat view the span from the first heatmap launch to the colour kernel, the chunks' synchronisations included), median over the
    window's calls after one warm-up call;
  * end-to-end frames/s of ``render.render_frames`` by the host clock (packing, copies both ways, the kernels; the call returns
    after the device synchronise): the lowest and highest of three windows of --window seconds.
Beside it, for context and not parity, the same detections drawn on the host on ONE frame: the NumPy restatement
(tests/render_reference.py; 10 detections only -- it blends full frames per primitive) and PIL ImageDraw (rectangles and
axis-aligned ellipses only, no labels).  The board's clocks and power as rocm-smi reports them are printed first."""
import argparse
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = [(720, 1280), (375, 1242)]
COUNTS = [10, 100]


def make_rows(seed, count, h, w):
    from bayes_od_rc_amd import render
    rng = np.random.RandomState(seed)
    bw, bh = rng.uniform(20, 240, count), rng.uniform(20, 200, count)
    x0, y0 = rng.uniform(0, w - bw), rng.uniform(0, h - bh)
    boxes = np.stack([x0, y0, x0 + bw, y0 + bh], axis=1).astype(np.int32)
    s = rng.uniform(1.0, 6.0, (count, 2, 2))
    rho = rng.uniform(-0.7, 0.7, (count, 2))
    covs = np.zeros((count, 2, 2, 2), np.float32)
    covs[:, :, 0, 0], covs[:, :, 1, 1] = s[:, :, 0] ** 2, s[:, :, 1] ** 2
    covs[:, :, 0, 1] = covs[:, :, 1, 0] = rho * s[:, :, 0] * s[:, :, 1]
    colors = np.asarray([render.PALETTE[i % len(render.PALETTE)] for i in range(count)], np.uint8)
    labels = ["%s %.2f" % (("car", "person", "truck")[i % 3], rng.uniform(0.5, 1)) for i in range(count)]
    return render.make_detections(boxes, covs, colors, labels)


class StderrCapture(object):
    """The library's trace lines go to the C stderr: route fd 2 through a file for the duration."""

    def __enter__(self):
        self.tmp = tempfile.TemporaryFile(mode="w+b")
        sys.stderr.flush()
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()


def measure(frames, dets, view, window):
    from bayes_od_rc_amd import render
    render.render_frames(frames, dets, view=view)                                # warm-up: code objects, first allocations
    os.environ["BOD_RENDER_TRACE"] = "1"
    with StderrCapture() as cap:
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < window / 2:
            render.render_frames(frames, dets, view=view)
    del os.environ["BOD_RENDER_TRACE"]
    ms = [[float(v) for v in re.findall(r"(?:bin|paint|colour) ([0-9.]+)", line)] for line in cap.text.splitlines() if line.startswith("# render_frames")]
    device = np.median(np.asarray(ms), axis=0)
    rates = []
    for _ in range(3):                                                           # three windows: the spread is part of the figure
        calls, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < window:
            render.render_frames(frames, dets, view=view)
            calls += 1
        rates.append(calls * len(frames) / (time.perf_counter() - t0))
    return device, (min(rates), max(rates))


def host_numpy(frame, det):
    import render_reference as ref
    from bayes_od_rc_amd import render
    font = render.font()
    t0 = time.perf_counter()
    ref.overlay(frame, det.boxes, det.corner_covs, det.colors, det.text, None, 2, True, render.R2_TWO_SIGMA, font)
    return time.perf_counter() - t0


def host_pil(frame, det):
    from PIL import Image, ImageDraw
    from bayes_od_rc_amd import render
    ImageDraw.Draw(Image.fromarray(frame)).rectangle([0, 0, 4, 4], outline=(1, 2, 3))     # first use loads PIL's drawing code
    t0 = time.perf_counter()
    im = Image.fromarray(frame)
    draw = ImageDraw.Draw(im)
    for box, covs, col in zip(det.boxes, det.corner_covs, det.colors):
        draw.rectangle([int(v) for v in box], outline=tuple(int(c) for c in col), width=1)
        for (cx, cy), c in zip(((box[0], box[1]), (box[2], box[3])), covs):
            rx, ry = (render.R2_TWO_SIGMA * c[0, 0]) ** 0.5, (render.R2_TWO_SIGMA * c[1, 1]) ** 0.5
            draw.ellipse([cx - rx, cy - ry, cx + rx, cy + ry], outline=tuple(int(v) for v in col), width=2)
    np.asarray(im)
    return time.perf_counter() - t0


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--heat-frames", type=int, default=4)
    ap.add_argument("--window", type=float, default=2.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    try:
        smi = subprocess.run(["rocm-smi", "--showclocks", "--showpower"], capture_output=True, text=True, timeout=60).stdout
        for l in smi.splitlines():
            if re.search(r"GPU\[0\].*(sclk|mclk|Power)", l):
                say("# " + l.strip())
    except Exception as e:                                                       # the figures stand without it
        say("# rocm-smi not available: %s" % e)
    say("size detections view frames device_ms_per_call(bin,paint | span) device_ms_per_frame frames_per_s_end_to_end")
    for h, w in SIZES:
        rng = np.random.RandomState(h)
        for count in COUNTS:
            for view in ("overlay", "heat"):
                n = args.frames if view == "overlay" else args.heat_frames
                frames = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(n)]
                dets = [make_rows(100 * count + i, count, h, w) for i in range(n)]
                device, fps = measure(frames, dets, view, args.window)
                say("%dx%d %d %s %d %s %.4f %.1f-%.1f" % (h, w, count, view, n, ",".join("%.4f" % v for v in device), device.sum() / n, fps[0], fps[1]))
        frame = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        say("%dx%d host, one frame: NumPy restatement 10 detections %.3f s; PIL ImageDraw (boxes and axis-aligned ellipses) 10 detections %.5f s, "
            "100 detections %.5f s" % (h, w, host_numpy(frame, make_rows(1, 10, h, w)), host_pil(frame, make_rows(1, 10, h, w)),
                                       host_pil(frame, make_rows(2, 100, h, w))))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fp:
            fp.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
