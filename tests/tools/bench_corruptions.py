"""Timing of the corruption stage (profiles/corruption_kernels.txt).

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 tests/tools/bench_corruptions.py kernels
    python3 tests/tools/bench_corruptions.py summary DIR        # per kernel: the launches' durations, median of three, byte floor
    python3 tests/tools/bench_corruptions.py upload             # upload_frames_u8_ragged with / without a defocus_blur:5 chain

``kernels`` runs every op three times through bod_corrupt_frames_u8 on 16 frames of 720x1280 (one op per call, so a kernel's
launches in the trace are that op's); the kernel times are the profiler's, since 16 frames are a few tens of microseconds and an
event pair around the stand-alone entry would time its copies.  Byte floor: 6 bytes per pixel (3 read, 3 written) at the 6.29 TB/s
a float4 copy measures.  ``upload`` with BOD_LIB_OVERRIDE naming another build of the library (one without the
corruption entries: the parent commit's) times the plain upload alone."""
import csv
import glob
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

N, H, W = 16, 720, 1280
HBM = 6.29e12


def frames():
    rng = np.random.RandomState(0)
    return [rng.randint(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(N)]


def ops():
    from bayes_od_rc_amd import corruptions as c
    return [("NONE (copy)", c.op_none()), ("LUT", c.op_lut(c.lut_gamma(2.0))), ("CONTRAST", c.op_contrast(0.5)),
            ("IMPULSE_NOISE", c.op_impulse_noise(0.1)), ("GAUSSIAN_NOISE", c.op_gaussian_noise(16.0)),
            ("CONV2D K=3", c.op_conv2d(c.gaussian_kernel(0.3))), ("CONV2D K=21", c.op_conv2d(c.disk_kernel(10.0))),
            ("CONV2D K=19 (defocus_blur:5)", c.make("defocus_blur", 5)), ("PIXELATE f=8", c.op_pixelate(8)),
            ("JPEG q=50", c.op_jpeg(50)), ("FOG", c.op_fog(160))]


def run_kernels():
    from bayes_od_rc_amd.engine import corrupt_frames
    fr = frames()
    for name, chain in ops():
        for _ in range(3):
            corrupt_frames(fr, chain, seed=1)
        print("ran", name, flush=True)


def summary(directory):
    paths = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    if not paths:
        raise SystemExit("no *kernel_trace.csv under %s" % directory)
    rows = []
    for p in paths:
        with open(p) as fp:
            rows += list(csv.DictReader(fp))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    floor_us = 6.0 * N * H * W / HBM * 1e6
    print("16 frames of 720x1280; byte floor of an op: %.1f us (6 B per pixel at 6.29 TB/s)" % floor_us)
    launches = [(r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3) for r in rows if "corrupt_" in r["Kernel_Name"]]
    names = [n for n, _ in ops()]
    # in launch order: three calls per op; CONTRAST is two kernels per call
    i = 0
    for name in names:
        per_call = 2 if name == "CONTRAST" else 1
        group = launches[i:i + 3 * per_call]
        i += 3 * per_call
        for k in range(per_call):
            durs = [group[c * per_call + k][1] for c in range(3)]
            kern = re.search(r"corrupt_\w+(<\d+>)?", group[k][0]).group(0)
            print("%-30s %-28s %s us, median %.1f us = %.1fx the floor" %
                  (name, kern, " / ".join("%.1f" % d for d in durs), float(np.median(durs)), float(np.median(durs)) / floor_us))
    assert i == len(launches), (i, len(launches))


def run_upload():
    from bayes_od_rc_amd import _lib
    override = bool(os.environ.get("BOD_LIB_OVERRIDE"))
    if override:                                       # a build without the corruption entries
        for name in ("bod_corrupt_frames_u8", "bod_set_upload_corruption"):
            _lib.SIGNATURES.pop(name, None)
    from bayes_od_rc_amd.engine import Engine, make_config
    fr = frames()
    eng = Engine(make_config((H, W), batch=N, mc_samples=2))
    chain = None
    if not override:
        from bayes_od_rc_amd import corruptions
        chain = corruptions.make("defocus_blur", 5)

    def timed(with_chain):
        t = []
        for _ in range(7):
            if with_chain:
                eng.set_upload_corruption(chain, seed=1)
            t0 = time.perf_counter()
            eng.upload_frames_u8_ragged(fr, aspect_resize=False)
            t.append((time.perf_counter() - t0) * 1e3)
        return t[2:]
    for rep in range(3):
        plain = timed(False)
        print("rep %d  upload_frames_u8_ragged, %d frames of %dx%d%s: median %.2f ms (%s)" %
              (rep, N, H, W, " [library: %s]" % os.environ["BOD_LIB_OVERRIDE"] if override else "", float(np.median(plain)),
               ", ".join("%.2f" % v for v in plain)), flush=True)
        if chain is not None:
            blur = timed(True)
            print("rep %d  the same with a defocus_blur:5 chain (CONV2D K=19):  median %.2f ms (%s)" %
                  (rep, float(np.median(blur)), ", ".join("%.2f" % v for v in blur)), flush=True)
    eng.close()


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "kernels":
        run_kernels()
    elif mode == "summary":
        summary(sys.argv[2])
    elif mode == "upload":
        run_upload()
    else:
        raise SystemExit(__doc__)
