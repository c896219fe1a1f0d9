"""Host sanitizer build of the PNG decoder's host half (bayes-od-rc_amd/csrc/png_inflate.h): the chunk parser and the
inflate compiled with -fsanitize=address,undefined into a stand-alone program (tests/host/png_inflate_check.cpp) that feeds them every
truncation prefix and every single-byte substitution by 0x00 / 0xFF of five small corpus files, one per deflate mode and colour type
-- each substitution also with its chunk's CRC-32 recomputed, and every prefix of the zlib stream as a well-formed file, so that the
inflate itself sees hostile input.  Every call must return PNG_OK or PNG_INVALID with the sanitizers silent; the intact files must
hash to the bytes zlib.decompress gives."""
import os
import shutil
import subprocess
import zlib

import png_corpus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fnv1a(data):
    h = 1469598103934665603
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def _pick(cases):
    """One file per deflate mode and colour type, small enough that six inputs per byte stay quick under the sanitizers."""
    want = [("stored", 0), ("level6", 2), ("level9", 4), ("fixed", 6), ("pil", 2)]
    picked = []
    for mode, color_type in want:
        fit = [c for c in cases if c.mode == mode and c.color_type == color_type and c.height * c.width >= 100 and len(c.data) <= 1200]
        assert fit, (mode, color_type)
        picked.append(max(fit, key=lambda c: len(c.data)))
    return picked


def test_png_inflate_under_asan_ubsan(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = str(tmp_path / "png_inflate_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
           "-I" + os.path.join(ROOT, "bayes-od-rc_amd", "csrc"), os.path.join(ROOT, "tests", "host", "png_inflate_check.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    args = []
    for i, c in enumerate(_pick(png_corpus.load())):
        path = tmp_path / ("case%d.png" % i)
        path.write_bytes(c.data)
        args += [str(path), "%016x" % _fnv1a(zlib.decompress(png_corpus.idat_stream(c.data)))]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe] + args, capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failures" in r.stdout, r.stdout
    print(r.stdout)
    tried = int(r.stdout.split("files,")[1].split()[0])
    assert tried >= 10000, r.stdout
    refused = int(r.stdout.split("decoded,")[1].split()[0])
    assert refused >= tried // 4, r.stdout            # the hostile inputs do reach the error paths


def test_engine_uses_the_checked_decoder():
    """engine.hip must decode with the header the sanitizer run checks, not with a private copy."""
    src = open(os.path.join(ROOT, "bayes-od-rc_amd", "csrc", "engine.hip")).read()
    assert '#include "png_inflate.h"' in src
    for fn in ("png_parse(", "png_decode("):
        assert fn in src, fn
    for private in ("png_inflate_blocks", "PngBits", "png_build_huff"):
        assert private not in src, private
