"""Host sanitizer build of the post stages' host bookkeeping (bayes-od-rc_amd/csrc/record_state.h, what engine.hip uses for the
record slots' staging layout, the stage state, the zero rows behind a detection count and the stage entry points' convolution
geometry): tests/host/record_state_check.cpp builds it under -fsanitize=address,undefined and checks the layout against the literal
formulas, the stage state against a four-bool restatement over every event sequence up to length 5, the zeroing for counts -1, 0,
1, K and K + 3, and the geometry for planes 1..9, kernels 1..3, strides 1 and 2, SAME and VALID."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bayes-od-rc_amd", "csrc")


def test_record_state_under_asan_ubsan(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = str(tmp_path / "record_state_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
           "-I" + CSRC, os.path.join(ROOT, "tests", "host", "record_state_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert "0 failures" in r.stdout, r.stdout
    # 48 layouts + (7 + 7^2 + ... + 7^5) stage events + 1 + 30 zeroings + 2 916 geometries
    assert int(r.stdout.split("record_state_check:")[1].split()[0]) == 48 + 19607 + 1 + 30 + 2916


def test_engine_uses_the_checked_header():
    """The engine must use what the sanitizer run checks and keep no copy of its own.  A tripwire on the source text only; that
    the device agrees is what tests/test_gpu_record_slots.py shows."""
    src = open(os.path.join(CSRC, "engine.hip")).read()
    assert '#include "record_state.h"' in src
    for gone in ("2 * C + 20", "select_slot", "auto done = [&](bod_status", "same_pad_before(int"):
        assert gone not in src, gone
    for used in ("RecordLayout", "StageState stage", "zero_rows_past_count(", "conv_out_geometry("):
        assert used in src, used
    train = open(os.path.join(CSRC, "train_impl.inc")).read()
    assert "struct StageScope" in src and "struct StageScope" not in train and "conv_out_geometry(" in train
    # one pack kernel, its field offsets from the header
    post = open(os.path.join(CSRC, "post_kernels.hip")).read()
    assert post.count("__global__ __launch_bounds__(256) void pack_records") == 1 and "record_fields(" in post
