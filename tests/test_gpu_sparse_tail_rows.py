"""The sparse tail on 192-row tiles (engine.hip build_plan: SparseTailArgs.tail_rows, ConvArgs.tile_rows; conv_igemm.hip: the tower
loop with three 16-row pixel fragments per wave, conv_igemm_kernel<256, 192, 2, 4, 0, true>).  The tail computes the same
(pixel, sample) rows with the same products in the same order, the same dropout draws and the same sample order in the MC
reduction whatever the tile height, so detections and posteriors of BOD_SPARSE_TAIL_ROWS=192 (the default), =256 (today's tiles)
and BOD_SPARSE_TAIL=0 (the dense plan) must be equal bit for bit.  Batch 2, a square frame and a non-square one whose pyramid widths
are not multiples of 4; per sample count the slot limit and the padding differ:
  N = 10: 19 slots, 190 rows, the last fragment partly padding;  N = 30: 6 slots, 180 rows;
  N = 2: 96 slots, all 192 rows valid, tiles closing on their slots;  N = 7: 27 slots, 189 rows;
a foreground bias that keeps every anchor (long runs, full tiles), one that keeps none (device-side tile count 0: every workgroup
exits) and one that keeps a handful.  With little kept, N = 2 tiles close on their extended rows half empty, so N = 2 also runs with
every anchor kept: whole pyramid rows as runs, tiles that close on their 96 slots with all 192 rows valid and no padding row.  That
case reads the engine's BOD_SPARSE_STATS line and holds the tile count and the number of full tiles against a replay of the packing
rule.  plan_info() reports the tile height.  The keep sets here are whatever the random network fires on; test_gpu_sparse_masks.py
chooses them through a class layer that ignores its input (a bias f keeps each pixel with one probability)."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCRIPT = r"""
import os, sys
import numpy as np
sys.path.insert(0, %(root)r)
from bayes_od_rc_amd import synthetic
from bayes_od_rc_amd.anchor_generator import FpnAnchorGenerator
from bayes_od_rc_amd.engine import Engine, make_config

ACFG = {"layers": [3, 4, 5, 6, 7], "aspect_ratios": [[1.0, 1.0], [1.0, 2.0], [2.0, 1.0]], "scales": [1.0, 1.26, 1.59]}
PLANS = ("192", "256", "dense")
WEIGHTS, ANCHORS = {}, {}

def engine(hw, b, n, bias, plan):
    os.environ["BOD_SPARSE_TAIL"] = "0" if plan == "dense" else "1"      # (read when the plan is built: with the weights)
    if plan != "dense":
        os.environ["BOD_SPARSE_TAIL_ROWS"] = plan
    try:
        if bias not in WEIGHTS:
            WEIGHTS[bias] = synthetic.make_weights(cls_fg_bias=bias)
        if hw not in ANCHORS:
            ANCHORS[hw] = FpnAnchorGenerator(ACFG).generate_all((hw[0], hw[1], 3))
        eng = Engine(make_config(hw, batch=b, mc_samples=n))
        eng.load_weights(WEIGHTS[bias])
        eng.set_anchors(ANCHORS[hw])
        info = eng.plan_info()
    finally:
        os.environ.pop("BOD_SPARSE_TAIL")
        os.environ.pop("BOD_SPARSE_TAIL_ROWS", None)
    assert info["aggregating"] and info["sparse_tail"] == (plan != "dense"), info
    assert info["sparse_tail_rows"] == (0 if plan == "dense" else int(plan)), info
    return eng

def same(tag, x, y):
    assert type(x) == type(y), tag
    if isinstance(x, dict):
        assert set(x) == set(y), tag
        for k in x:
            same(tag + "." + k, x[k], y[k])
    elif isinstance(x, (tuple, list)):
        assert len(x) == len(y), tag
        for i, (u, v) in enumerate(zip(x, y)):
            same("%%s[%%d]" %% (tag, i), u, v)
    else:
        u, v = np.asarray(x), np.asarray(y)
        assert u.shape == v.shape and u.dtype == v.dtype, (tag, u.shape, v.shape)
        assert np.array_equal(u.view(np.uint8), v.view(np.uint8)), tag

def outputs(eng):
    return {"kept": eng.num_kept(), "post": [eng.get_posterior(i) for i in range(eng.B)],
            "det": [eng.get_detections(i) for i in range(eng.B)]}

def case(tag, hw, n, bias):
    frames = synthetic.make_frames(2, hw[0], hw[1], seed=5)
    outs = []
    for plan in PLANS:
        eng = engine(hw, 2, n, bias, plan)
        eng.infer(frames, seed=77, first_image_id=3)
        outs.append(outputs(eng))
        eng.close()
    for plan, o in zip(PLANS[1:], outs[1:]):
        same(tag + ":192 vs " + plan, outs[0], o)
    print(tag, "kept", outs[0]["kept"].tolist(), flush=True)
    return outs[0]["kept"]

SQUARE, ODD = (128, 128), (136, 200)          # pyramid widths 16 8 4 2 1 and 25 13 7 4 2
ANCHORS_PER_IMAGE = {SQUARE: 9 * (256 + 64 + 16 + 4 + 1), ODD: 9 * (17 * 25 + 9 * 13 + 5 * 7 + 3 * 4 + 2 * 2)}
which = sys.argv[1]
if which.startswith("n"):
    n = int(which[1:])
    for name, hw in (("square", SQUARE), ("nonsquare", ODD)):
        k = case("%%s_n%%d" %% (name, n), hw, n, -3.2)
        assert k.sum() > 0, k
elif which == "keep_all":
    for name, hw in (("square", SQUARE), ("nonsquare", ODD)):
        k = case("keep_all_" + name, hw, 10, 40.0)
        assert (k == ANCHORS_PER_IMAGE[hw]).all(), (k, ANCHORS_PER_IMAGE[hw])
elif which == "keep_all_n2":
    for name, hw in (("square", SQUARE), ("nonsquare", ODD)):
        k = case("keep_all_n2_" + name, hw, 2, 40.0)
        assert (k == ANCHORS_PER_IMAGE[hw]).all(), (k, ANCHORS_PER_IMAGE[hw])
elif which == "keep_none":
    k = case("keep_none", ODD, 10, -40.0)
    assert (k == 0).all(), k
elif which == "keep_few":
    k = case("keep_few", ODD, 10, %(few_bias)r)
    assert 0 < k.sum() <= 40, k
print("DONE", flush=True)
"""

# the foreground bias at which the synthetic weights keep a handful of the non-square frames' anchors (8 and 5 of 5 337; -3.2 keeps 58 each, -4.5 none)
FEW_BIAS = -4.0


def _run(which, **extra_env):
    env = dict(os.environ, BOD_FORCE_CONV_TILE="256", **extra_env)
    env.pop("BOD_SPARSE_TAIL_ROWS", None)
    r = subprocess.run([sys.executable, "-c", SCRIPT % {"root": ROOT, "few_bias": FEW_BIAS}, which], env=env, capture_output=True, text=True, timeout=600)
    print(r.stdout[-1500:])
    assert r.returncode == 0 and "DONE" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    return r


@pytest.mark.parametrize("which", ["n10", "n30", "n2", "n7", "keep_all", "keep_none", "keep_few"])
def test_tail_on_192_row_tiles_is_bit_identical_to_256_and_dense(which):
    _run(which)


def _packed_tiles(widths_heights, n, rows, ext_rows=320):
    """(tiles, tiles with all `rows` rows valid) of one image with every pixel kept: the runs are the whole rows of each pyramid level,
    packed by the rule of sparse_tables.h st_pack_run -- a piece of `take` pixels costs n * (take + 2) extended rows, a tile closes
    when its rows / n slots are full or no piece of one pixel fits any more."""
    qmax = rows // n
    tiles = full = 0
    q = x = 0
    is_open = False
    for w, h in widths_heights:
        for _ in range(h):
            left = w
            while left > 0:
                if not is_open:
                    q, x, is_open = 0, 0, True
                take = min(left, qmax - q, (ext_rows - x) // n - 2)
                if take < 1:
                    tiles += 1; full += q * n == rows; is_open = False
                    continue
                x += n * (take + 2); q += take; left -= take
                if q == qmax:
                    tiles += 1; full += q * n == rows; is_open = False
    if is_open:
        tiles += 1; full += q * n == rows
    return tiles, full


def test_n2_with_everything_kept_runs_tiles_without_a_padding_row():
    """N = 2, every anchor kept: tiles close on their 96 slots (128 on 256-row tiles) and have no padding row; the device's table has
    exactly the tiles and full tiles of the packing rule, and the three plans agree bit for bit."""
    r = _run("keep_all_n2", BOD_SPARSE_STATS="1")
    got = [(int(m.group(2)), int(m.group(1)), int(m.group(3))) for m in
           re.finditer(r"BOD_SPARSE_STATS: tail (\d+) tiles of (\d+) rows, .*?, (\d+) tiles with all \2 rows valid", r.stderr)]
    levels = {"square": [(16, 16), (8, 8), (4, 4), (2, 2), (1, 1)], "nonsquare": [(25, 17), (13, 9), (7, 5), (4, 3), (2, 2)]}
    want = []
    for name in ("square", "nonsquare"):             # the order the script runs them in; per geometry the 192- then the 256-row plan
        for rows in (192, 256):
            tiles, full = _packed_tiles(levels[name], 2, rows)
            assert full >= 2 and full >= tiles - 1, (name, rows, tiles, full)        # every tile but an image's last is full
            want.append((rows, 2 * tiles, 2 * full))                                 # batch 2, same geometry
    assert got == want, (got, want, r.stderr[-2000:])
