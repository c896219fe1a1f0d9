"""Host sanitizer build of the sparse tail / halo row-table builder (bayes-od-rc_amd/csrc/sparse_tables.h, the rules
sparse_tail_rows_kernel runs on the device): tests/host/sparse_tables_check.cpp replays the kernel's phases on the CPU under
-fsanitize=address,undefined and checks them against the serial walk they replaced and against brute-force 3x3 dilation."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sparse_tables_under_asan_ubsan(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = str(tmp_path / "sparse_tables_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
           "-I" + os.path.join(ROOT, "bayes-od-rc_amd", "csrc"), os.path.join(ROOT, "tests", "host", "sparse_tables_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert "0 failures" in r.stdout, r.stdout
    assert int(r.stdout.split("sparse_tables_check:")[1].split()[0]) >= 90


def test_kernel_uses_the_checked_rules():
    """post_kernels.hip must build the tables with the functions the sanitizer run checks, not with a private copy."""
    src = open(os.path.join(ROOT, "bayes-od-rc_amd", "csrc", "post_kernels.hip")).read()
    for fn in ("st_member(", "st_dilated(", "st_run_edge(", "st_pack_run(", "st_pack_close(", "st_write_piece(", "st_pad_row(",
               "st_pad_ext("):
        assert fn in src, fn
