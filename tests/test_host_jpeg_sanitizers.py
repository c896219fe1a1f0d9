"""Host sanitizer build of the JPEG decoder's host half (bayes-od-rc_amd/csrc/jpeg_entropy.h): the parser and the
Huffman decoder compiled with -fsanitize=address,undefined into a stand-alone program (tests/host/jpeg_entropy_check.cpp) that feeds
them every truncation prefix and every single-byte substitution by 0x00 / 0xFF / 0xD9 of a handful of corpus files.  Every call must
return JPEG_OK or JPEG_INVALID with the sanitizers silent; the intact files must decode to the coefficients of the NumPy
restatement (tests/jpeg_reference.py)."""
import os
import shutil
import subprocess

import numpy as np

import jpeg_corpus
import jpeg_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fnv1a(data):
    h = 1469598103934665603
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def _pick(cases):
    """One file per sampling and one per variant, small enough that four inputs per byte stay quick under the sanitizers."""
    want = [("4:2:0", "restart"), ("4:2:2", "optimize"), ("4:4:4", "plain"), ("gray", "restart"), ("4:2:0", "optimize")]
    picked = []
    for sampling, variant in want:
        fit = [c for c in cases if c.sampling == sampling and c.variant == variant and c.width * c.height >= 64 and len(c.data) <= 1500]
        assert fit, (sampling, variant)
        picked.append(max(fit, key=lambda c: len(c.data)))
    return picked


def test_jpeg_entropy_decoder_under_asan_ubsan(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = str(tmp_path / "jpeg_entropy_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
           "-I" + os.path.join(ROOT, "bayes-od-rc_amd", "csrc"), os.path.join(ROOT, "tests", "host", "jpeg_entropy_check.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    cases, _ = jpeg_corpus.load()
    args = []
    for i, c in enumerate(_pick(cases)):
        path = tmp_path / ("case%d.jpg" % i)
        path.write_bytes(c.data)
        coefs, _, _ = jpeg_reference.entropy_decode(c.data)
        args += [str(path), "%016x" % _fnv1a(np.ascontiguousarray(coefs, "<i2").tobytes())]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe] + args, capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failures" in r.stdout, r.stdout
    tried = int(r.stdout.split("files,")[1].split()[0])
    assert tried >= 10000, r.stdout
    refused = int(r.stdout.split("decoded,")[1].split()[0])
    assert refused >= tried // 4, r.stdout            # the hostile inputs do reach the error paths


def test_engine_uses_the_checked_decoder():
    """engine.hip must decode with the header the sanitizer run checks, not with a private copy."""
    src = open(os.path.join(ROOT, "bayes-od-rc_amd", "csrc", "engine.hip")).read()
    assert '#include "jpeg_entropy.h"' in src
    for fn in ("jpeg_parse(", "jpeg_decode("):
        assert fn in src, fn
