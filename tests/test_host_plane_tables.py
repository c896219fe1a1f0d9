"""Host sanitizer build of the plane -> plane row tables with an output step (bayes-od-rc_amd/csrc/plane_tables.h, what engine.hip's
make_table calls): tests/host/plane_tables_check.cpp builds the step-2 table of a stage's last `2c` under
-fsanitize=address,undefined for planes 128x128, 25x19, 13x10, 7x5 and 1x1 at batch 1 and 3 and checks its row count, each row
against the dense table's row of pixel (2y, 2x), the written pixels against what the next stage's stride-2 VALID 1x1 table reads,
and the even-row tiling of stage 4's `2b`."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stage_end_tables_under_asan_ubsan(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = str(tmp_path / "plane_tables_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
           "-I" + os.path.join(ROOT, "bayes-od-rc_amd", "csrc"), os.path.join(ROOT, "tests", "host", "plane_tables_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert "0 failures" in r.stdout, r.stdout
    # 5 planes x 2 batch sizes
    assert int(r.stdout.split("plane_tables_check:")[1].split()[0]) == 10


def test_engine_builds_its_tables_with_the_checked_function():
    """make_table must call the function the sanitizer run checks.  A tripwire on the source text only; that the device runs the
    step-2 tables is what tests/test_gpu_stage_end_pixels.py shows (M of the three `2c` ops, results bit-identical to the whole planes)."""
    src = open(os.path.join(ROOT, "bayes-od-rc_amd", "csrc", "engine.hip")).read()
    assert '#include "plane_tables.h"' in src
    assert "plane_row_table(B, gi, go, stride, org_y, org_x" in src
    assert "plane_rows_of_even_y(" in src
    assert "plane_step_view(dense)" in src and "PLANE_STEP_VIEW_BYTES" in src
