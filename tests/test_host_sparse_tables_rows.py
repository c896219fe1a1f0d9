"""Host sanitizer build of the sparse tail's row table at 192 and 256 rows per tile (bayes-od-rc_amd/csrc/sparse_tables.h, the `R`
parameter the device kernel passes from SparseTailArgs.tail_rows): tests/host/sparse_tables_rows_check.cpp replays the kernel's
phases on the CPU under -fsanitize=address,undefined and checks them against a serial walk with slot limit R / N, the row-reuse
invariants, the capacity bound for N in {2, 7, 10, 30, 64}, and the tile count of the 192-row table against the 256-row one."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sparse_tail_rows_tables_under_asan_ubsan(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = str(tmp_path / "sparse_tables_rows_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
           "-I" + os.path.join(ROOT, "bayes-od-rc_amd", "csrc"), os.path.join(ROOT, "tests", "host", "sparse_tables_rows_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert "0 failures" in r.stdout, r.stdout
    # 5 sample counts x 5 geometries x 6 densities x 2 heights
    assert int(r.stdout.split("sparse_tables_rows_check:")[1].split()[0]) == 300
    # one line per sample count with the tile counts at the 0.18 density (the 2 % bound itself is checked by the program)
    assert len(re.findall(r"^N=\d+ density 0\.18: \d+ tiles of 192 rows, \d+ of 256", r.stdout, flags=re.M)) == 5


def test_kernel_passes_the_tile_height_to_the_checked_rules():
    """sparse_tail_rows_kernel must hand the tail's tile height to the functions the sanitizer run checks.  A tripwire on the source
    text only; that the device builds the 192-row table by these rules is what tests/test_gpu_sparse_tail_rows.py shows (tile and
    full-tile counts against a replay of the packing rule, and results bit-identical to the 256-row and dense plans)."""
    src = open(os.path.join(ROOT, "bayes-od-rc_amd", "csrc", "post_kernels.hip")).read()
    assert re.search(r"st_pack_run\([^;]*\bR\)", src)
    assert re.search(r"st_write_piece\([^;]*\bR\)", src)
    assert "a.tail_rows" in src
