"""Pins the Python restatement of the sparse tail / halo tables (tests/sparse_tables_reference.py) to the header the kernel runs
(bayes-od-rc_amd/csrc/sparse_tables.h): tests/host/sparse_tables_dump.cpp, built with -fsanitize=address,undefined and run directly,
prints the flags, runs, pieces and tiles the header's functions make of a mask, and they must EQUAL the restatement's -- both tables,
tail tiles of 192 and 256 rows, N = 2, 7, 10, 30, the 128x128 and the 136x200 frames' pyramids, Bernoulli masks at four densities and
hand-made masks at the borders of the rules (gaps, row ends that touch row starts, the levels at most 4 wide, ...)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import sparse_tables_reference as st

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LEVEL_SETS = {"square": st.SQUARE_LEVELS, "odd": st.ODD_LEVELS}
SAMPLES = (2, 7, 10, 30)
TAIL_ROWS = (192, 256)
DENSITIES = (0.01, 0.1, 0.5, 0.95)


def _level_slices(levels):
    out, p = [], 0
    for w, h in levels:
        out.append((p, w, h))
        p += w * h
    return out


def hand_made_masks(levels):
    p = st.num_pixels(levels)
    masks = {"nothing": np.zeros(p, bool), "everything": np.ones(p, bool)}
    for name, idx in (("pixel_0", [0]), ("pixel_last", [p - 1])):
        masks[name] = np.zeros(p, bool)
        masks[name][idx] = True
    idx = np.arange(p)
    masks["every_second_pixel"] = idx % 2 == 0
    masks["every_third_pixel"] = idx % 3 == 0
    corners, rows2, cols, narrow = (np.zeros(p, bool) for _ in range(4))
    for p0, w, h in _level_slices(levels):
        v = lambda m: m[p0:p0 + w * h].reshape(h, w)            # (a view: writes land in m)
        for y in (0, h - 1):
            for x in (0, w - 1):
                v(corners)[y, x] = True
        v(rows2)[::2, :] = True
        v(cols)[:, 0] = True
        v(cols)[:, w - 1] = True
        if w <= 4:
            v(narrow)[...] = True
    masks.update(corners=corners, every_second_row=rows2, first_and_last_column=cols, narrow_levels=narrow)
    return masks


def all_masks(levels, key):
    masks = hand_made_masks(levels)
    rng = np.random.default_rng(2024 + key)
    for d in DENSITIES:
        masks["bernoulli_%g" % d] = rng.random(st.num_pixels(levels)) < d
    return masks


@pytest.fixture(scope="module")
def dump_exe(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = str(tmp_path_factory.mktemp("sparse_tables_dump") / "sparse_tables_dump")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
           "-I" + os.path.join(ROOT, "bayes-od-rc_amd", "csrc"), os.path.join(ROOT, "tests", "host", "sparse_tables_dump.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _run_dump(exe, path):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, path], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-3000:])
    return r.stdout


def _parse(text):
    """[{"P", "min_pixels", "min_pixels_tail", "flags", "tables": [{"runs", "pieces", "tiles"}] * 2}] from the program's output"""
    cases = []
    for line in text.splitlines():
        word, *rest = line.split()
        if word == "case":
            cases.append({"P": int(rest[0]), "min_pixels": int(rest[1]), "min_pixels_tail": int(rest[2]), "tables": []})
        elif word == "flags":
            cases[-1]["flags"] = np.array([int(c, 16) for c in rest[0]], np.uint8)
        elif word == "table":
            assert int(rest[0]) == len(cases[-1]["tables"])
            cases[-1]["tables"].append({"counts": tuple(int(x) for x in rest[1:]), "runs": [], "pieces": [], "tiles": []})
        else:
            cases[-1]["tables"][-1][word + "s"].append(tuple(int(x) for x in rest))
    return cases


@pytest.mark.parametrize("geometry", sorted(LEVEL_SETS))
def test_restatement_equals_the_header(dump_exe, tmp_path, geometry):
    levels = LEVEL_SETS[geometry]
    p = st.num_pixels(levels)
    masks = all_masks(levels, len(geometry))
    assert len(masks) == 14
    wanted, lines = [], []
    for n in SAMPLES:
        for rows in TAIL_ROWS:
            for name, mask in masks.items():
                wanted.append((n, rows, name, mask))
                lines.append("%d %d %d  %s\n%s\n" % (len(levels), n, rows, " ".join("%d %d" % wh for wh in levels),
                                                     "".join("1" if k else "0" for k in mask)))
    path = str(tmp_path / "cases.txt")
    with open(path, "w") as f:
        f.writelines(lines)
    got = _parse(_run_dump(dump_exe, path))
    assert len(got) == len(wanted) == 4 * 2 * 14
    for (n, rows, name, mask), g in zip(wanted, got):
        tag = (geometry, n, rows, name)
        ref = st.tables(levels, mask, n, rows)
        assert g["P"] == p, tag
        assert g["min_pixels"] == st.min_pixels_per_closed_tile(n) == g["min_pixels_tail"] == st.min_pixels_per_closed_tile(n, rows), tag
        assert np.array_equal(g["flags"], ref["flags"]), (tag, g["flags"], ref["flags"])
        for t, which in enumerate(("tail", "halo")):
            r, d = ref[which], g["tables"][t]
            assert d["counts"] == (len(r["runs"]), len(r["pieces"]), len(r["tiles"])), (tag, which)
            assert d["runs"] == r["runs"], (tag, which)
            assert d["pieces"] == r["pieces"], (tag, which)
            assert d["tiles"] == [tile[:3] for tile in r["tiles"]], (tag, which)
            # the capacity the engine sizes its buffers by (every third pixel is the mask with the most extended rows per kept pixel)
            assert len(r["tiles"]) <= st.tile_capacity(levels, n) == p // g["min_pixels"] + 1, (tag, which)
            # the summary is the table's: valid rows = N per member pixel, full tiles = no padding row
            assert r["summary"]["valid_rows"] == n * sum(k for *_, k in d["pieces"]), (tag, which)
            assert r["summary"]["full_tiles"] == sum(1 for tile in d["tiles"] if tile[1] * n == r["rows"]), (tag, which)


def test_the_masks_are_what_their_names_say():
    """The hand-made masks reach the rules they are there for (on the restatement, which the test above pins to the header)."""
    levels = st.ODD_LEVELS
    p = st.num_pixels(levels)
    m = hand_made_masks(levels)
    t = {name: st.tables(levels, mask, 10, 192) for name, mask in m.items()}
    assert t["nothing"]["tail"]["summary"]["tiles"] == t["nothing"]["halo"]["summary"]["tiles"] == 0
    assert [r for r in t["everything"]["tail"]["runs"]] == [(p0 + y * w, w) for p0, w, h in _level_slices(levels) for y in range(h)]
    assert t["pixel_0"]["tail"]["runs"] == [(0, 1)] and t["pixel_0"]["halo"]["runs"] == [(0, 2), (25, 2)]
    assert t["pixel_last"]["tail"]["runs"] == [(p - 1, 1)] and t["pixel_last"]["halo"]["runs"] == [(p - 4, 2), (p - 2, 2)]
    # every second pixel: every gap is filled in rows of odd width (x = 0, 2, .., w - 1), the flat pattern leaves pairs elsewhere
    assert st.filled_gaps(t["every_second_pixel"]["flags"]) > 100
    # every third pixel: nothing filled, all runs one pixel long, every tile but the last closes on its extended rows
    third = t["every_third_pixel"]
    assert st.filled_gaps(third["flags"]) == 0 and all(k == 1 for _, k in third["tail"]["runs"])
    assert [tile[3] for tile in third["tail"]["tiles"][:-1]] == ["ext"] * (len(third["tail"]["tiles"]) - 1) and len(third["tail"]["tiles"]) > 10
    # first and last column: a run ends at a row's last pixel and the next pixel starts one -- two runs, never one across the row end
    cols = t["first_and_last_column"]["tail"]["runs"]
    assert (24, 1) in cols and (25, 1) in cols
    assert (p - 4, 2) in cols and (p - 2, 2) in cols            # the 2-wide level: both columns, one run per row
    # the levels at most 4 wide, whole: their dilation and gap fill meet both borders
    narrow = t["narrow_levels"]
    assert narrow["tail"]["runs"] == [(577, 4), (581, 4), (585, 4), (589, 2), (591, 2)] == narrow["halo"]["runs"]
    assert len(t["corners"]["tail"]["runs"]) == 4 * 5 - 2             # (the 2x2 level's corners pair up into two runs of two)
