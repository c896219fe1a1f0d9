"""The sparse tail and its halo on keep sets the test chooses (engine.hip build_plan; post_kernels.hip sparse_tail_rows_kernel;
sparse_tables.h; conv_igemm.hip's tower loop over the tables).  The other sparse tests take whatever a random network keeps; here the
class output layer ignores its input (sparse_tables_reference.lever_weights: zero kernel, a bias that gives class 0 of anchor type 0
the logit f), so post_sample_kernel keeps every pixel independently with one probability set by f, and every (seed, first_image_id)
of a call is another set of masks on the same engines.  Box and covariance towers keep their random weights.

Per case four engines -- the default plan (halo, 192-row tail tiles), BOD_SPARSE_TAIL_ROWS=256, BOD_SPARSE_HALO=0 and the dense plan
BOD_SPARSE_TAIL=0 -- run the same calls, and per call
  - num_kept, every image's posterior (anchor_index included) and detections are equal as bytes across the four plans; after the first
    call a posterior under another seed (the raw re-run) is equal across the three sparse plans;
  - the keep set read back from the dense plan has the property the case is there for (tiles closing on extended rows, filled gaps,
    more than 64 runs, ...): conditions on the device's masks, which f and the seeds were chosen on the host to meet with room;
  - each sparse plan's BOD_SPARSE_STATS line equals the Python replay (sparse_tables_reference.tables) of the DEVICE's masks summed
    over the batch -- tail tiles, valid tail rows, tail tiles with all rows valid, halo tiles -- and stays within its capacity.
The predicted figures (host twin of the categorical draws) are printed beside the device's, never asserted."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import sparse_tables_reference as st

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCRIPT = r"""
import json, os, sys
import numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, "tests"))
from bayes_od_rc_amd import synthetic
from bayes_od_rc_amd.anchor_generator import FpnAnchorGenerator
from bayes_od_rc_amd.engine import Engine, make_config
import sparse_tables_reference as st

ACFG = {"layers": [3, 4, 5, 6, 7], "aspect_ratios": [[1.0, 1.0], [1.0, 2.0], [2.0, 1.0]], "scales": [1.0, 1.26, 1.59]}
PLANS = {"default": {}, "rows256": {"BOD_SPARSE_TAIL_ROWS": "256"}, "nohalo": {"BOD_SPARSE_HALO": "0"}, "dense": {"BOD_SPARSE_TAIL": "0"}}
SWITCHES = ("BOD_SPARSE_TAIL", "BOD_SPARSE_TAIL_ROWS", "BOD_SPARSE_HALO")

def engine(hw, b, n, weights, anchors, plan):
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(PLANS[plan])                    # (read when the plan is built: with the weights)
    try:
        eng = Engine(make_config(hw, batch=b, mc_samples=n))
        eng.load_weights(weights)
        eng.set_anchors(anchors)
        info = eng.plan_info()
    finally:
        for k in SWITCHES:
            os.environ.pop(k, None)
    assert info["aggregating"] and info["sparse_tail"] == (plan != "dense"), (plan, info)
    assert info["sparse_halo"] == (plan in ("default", "rows256")), (plan, info)
    assert info["sparse_tail_rows"] == {"default": 192, "rows256": 256, "nohalo": 192, "dense": 0}[plan], (plan, info)
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

case = json.loads(sys.argv[1])
hw, b, n = tuple(case["hw"]), case["batch"], case["n"]
weights = st.lever_weights(synthetic.make_weights(), case["f"])
anchors = FpnAnchorGenerator(ACFG).generate_all((hw[0], hw[1], 3))
frames = synthetic.make_frames(b, hw[0], hw[1], seed=5)
engines = {plan: engine(hw, b, n, weights, anchors, plan) for plan in PLANS}
for i, (seed, first) in enumerate(case["calls"]):
    outs = {}
    for plan, eng in engines.items():
        sys.stderr.write("CALL %%d %%s\n" %% (i, plan)); sys.stderr.flush()       # (the engine's statistics line follows on stderr)
        eng.infer(frames, seed=seed, first_image_id=first)
        outs[plan] = outputs(eng)
    for plan in PLANS:
        same("call %%d: default vs %%s" %% (i, plan), outs["default"], outs[plan])
    if i == 0:
        # a posterior under another seed and first image: other anchors' statistics, which the sparse plans serve from the raw re-run
        # (the dense plan from its aggregated statistics: compared between the sparse plans, as test_gpu_sparse_halo.py does)
        post2 = {}
        for plan in ("default", "rows256", "nohalo"):
            engines[plan].posterior(seed=seed + 1000, first_image_id=first + 2)
            post2[plan] = [engines[plan].get_posterior(k) for k in range(b)]
        for plan in ("rows256", "nohalo"):
            same("posterior under another seed: default vs " + plan, post2["default"], post2[plan])
    print("MASKS", json.dumps({"call": i, "anchor_index": [p["anchor_index"].tolist() for p in outs["dense"]["post"]],
                               "kept": outs["dense"]["kept"].tolist()}), flush=True)
for eng in engines.values():
    eng.close()
print("DONE", flush=True)
"""

BATCH = 3
SQUARE, ODD = (128, 128), (136, 200)          # pyramid widths 16 8 4 2 1 and 25 13 7 4 2: all five levels, one not a multiple of 4 wide
LEVELS = {SQUARE: st.SQUARE_LEVELS, ODD: st.ODD_LEVELS}
CALLS = [(77, 3), (5000000011, 40)]                   # (the second seed has bits above 2^32)
# isolated pixels: calls, of seeds 70..129 x first images 3, 5, 40, whose predicted masks have >= 86 % one-pixel runs in every image,
# >= 5 tail tiles per image at both tile heights and no tile closed on its slots (the search is a loop over
# sparse_tables_reference.predicted_pixel_masks and .tables)
ISOLATED_CALLS = [(76, 5), (91, 40)]
# edges: sparse_tables_reference.find_edge_calls(EDGE_F, ODD_LEVELS) (its docstring says what each key stands for).  No device-side
# draw on the CDF's edge has broken one so far: the device's masks equalled the predicted ones pixel for pixel.
EDGE_CALLS = {"nothing": (131, 100), "coarse": (335, 100), "ends": (776, 100)}

# every f is exact in bfloat16; the density is sparse_tables_reference.keep_probability(f)
CASES = {
    "isolated_pixels": dict(hw=ODD, n=10, f=-0.5625, calls=ISOLATED_CALLS),                 # 0.087
    "mixed": dict(hw=ODD, n=10, f=0.0, calls=CALLS),                                        # 0.57
    "many_tiles": dict(hw=SQUARE, n=30, f=0.0, calls=CALLS),
    "long_tiles": dict(hw=ODD, n=2, f=0.0, calls=CALLS),
    "n_does_not_divide_the_tile": dict(hw=SQUARE, n=7, f=-0.5, calls=CALLS),                # 0.117
    "edges": dict(hw=ODD, n=10, f=st.EDGE_F, calls=list(EDGE_CALLS.values())),              # 0.011
}

STATS = re.compile(r"BOD_SPARSE_STATS: tail (\d+) tiles of (\d+) rows, [\d.]+ valid rows per tile \((\d+) rows = [\d.]+ of the dense launch's\), "
                   r"(\d+) tiles with all (\d+) rows valid; halo (\d+) tiles of 256 rows; dense plain tiles \d+; capacity (\d+) tiles")
PLAN_ROWS = {"default": 192, "rows256": 256, "nohalo": 192}


def _run(case):
    env = dict(os.environ, BOD_FORCE_CONV_TILE="256", BOD_SPARSE_STATS="1")
    for k in ("BOD_SPARSE_TAIL", "BOD_SPARSE_TAIL_ROWS", "BOD_SPARSE_HALO"):
        env.pop(k, None)
    arg = json.dumps(dict(case, batch=BATCH))
    r = subprocess.run([sys.executable, "-c", SCRIPT % {"root": ROOT}, arg], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "DONE" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    masks = [json.loads(line[6:]) for line in r.stdout.splitlines() if line.startswith("MASKS ")]
    assert [m["call"] for m in masks] == list(range(len(case["calls"])))
    stats, where = {}, None                        # (call, plan) -> the statistics line printed behind its marker
    for line in r.stderr.splitlines():
        if line.startswith("CALL "):
            where = (int(line.split()[1]), line.split()[2])
        elif line.startswith("BOD_SPARSE_STATS"):
            m = STATS.match(line)
            assert m and where is not None and where not in stats, (line, where)
            stats[where] = dict(zip(("tail_tiles", "rows", "valid_rows", "full_tiles", "rows2", "halo_tiles", "capacity"), map(int, m.groups())))
    return masks, stats


def _check_call(name, case, i, device, stats):
    """Replays the device's masks of call i, holds the three sparse plans' statistics lines against the replay, and returns
    [image][tile rows] -> tables for the property checks."""
    levels, n = LEVELS[case["hw"]], case["n"]
    seed, first = case["calls"][i]
    kept = []
    for b, idx in enumerate(device["anchor_index"]):
        idx = np.asarray(idx, np.int64)
        assert len(idx) == device["kept"][b]
        assert (idx % 9 == 0).all(), "only anchor type 0 can be kept with these weights"
        kept.append(st.pixel_mask(idx, levels))
    predicted = st.predicted_pixel_masks(case["f"], seed, first, BATCH, levels)
    replay = [{rows: st.tables(levels, k, n, rows) for rows in (192, 256)} for k in kept]
    guess = [{rows: st.tables(levels, k, n, rows) for rows in (192, 256)} for k in predicted]
    for what, masks, tabs in (("device", kept, replay), ("predicted", predicted, guess)):
        print("%s call %d seed %d first image %d %s: density %s, tail runs %s (one pixel: %s), tail tiles 192/256 %s / %s, halo tiles %s" % (
            name, i, seed, first, what, ["%.3f" % m.mean() for m in masks], [len(t[192]["tail"]["runs"]) for t in tabs],
            [sum(1 for _, k in t[192]["tail"]["runs"] if k == 1) for t in tabs], [len(t[192]["tail"]["tiles"]) for t in tabs],
            [len(t[256]["tail"]["tiles"]) for t in tabs], [len(t[256]["halo"]["tiles"]) for t in tabs]))
    print("%s call %d: %d pixels differ from the prediction" % (name, i, int(sum((k != p).sum() for k, p in zip(kept, predicted)))))
    for plan, rows in PLAN_ROWS.items():
        got = stats[(i, plan)]
        tail = [t[rows]["tail"]["summary"] for t in replay]
        want = {"tail_tiles": sum(s["tiles"] for s in tail), "rows": rows, "rows2": rows,
                "valid_rows": sum(s["valid_rows"] for s in tail), "full_tiles": sum(s["full_tiles"] for s in tail),
                "halo_tiles": 0 if plan == "nohalo" else sum(t[rows]["halo"]["summary"]["tiles"] for t in replay),
                "capacity": BATCH * st.tile_capacity(levels, n)}
        assert got == want, (name, i, plan, got, want)
        assert got["tail_tiles"] <= got["capacity"] and got["halo_tiles"] <= got["capacity"], (name, i, plan, got)
        for t in replay:                            # per image too: the kernel's scratch and the bound are per image
            assert len(t[rows]["tail"]["tiles"]) <= st.tile_capacity(levels, n) >= len(t[rows]["halo"]["tiles"])
    return kept, replay


def _closed(table, why):
    return sum(1 for t in table["tiles"] if t[3] == why)


def _properties(name, case, kept_calls, replay_calls):
    """The conditions each case is there for, on the device's masks."""
    levels, n = LEVELS[case["hw"]], case["n"]
    p = st.num_pixels(levels)
    images = [t for call in replay_calls for t in call]
    masks = [k for call in kept_calls for k in call]
    if name == "isolated_pixels":
        for t in images:
            runs = t[192]["tail"]["runs"]
            assert sum(1 for _, k in runs if k == 1) >= 0.8 * len(runs), runs
            for rows in (192, 256):
                assert _closed(t[rows]["tail"], "slots") == 0 and len(t[rows]["tail"]["tiles"]) >= 4
                assert _closed(t[rows]["tail"], "ext") == len(t[rows]["tail"]["tiles"]) - 1
    elif name == "mixed":
        assert max(len(t[192]["tail"]["runs"]) for t in images) > 64
        for call in replay_calls:                  # both closing rules in one call's table
            assert sum(_closed(t[192]["tail"], "slots") for t in call) > 0 and sum(_closed(t[192]["tail"], "ext") for t in call) > 0
        assert min(st.filled_gaps(t[192]["flags"]) for t in images) >= 1
    elif name == "many_tiles":
        assert 192 // n == 6
        for t in images:
            assert len(t[192]["tail"]["tiles"]) >= 30 and max(x[1] for x in t[192]["tail"]["tiles"]) == 6
            assert len(t[256]["halo"]["tiles"]) >= 30
    elif name == "long_tiles":
        assert 192 // n == 96
        for t in images:
            tail = t[192]["tail"]
            assert _closed(tail, "slots") >= 2 and tail["summary"]["full_tiles"] >= 2          # 96 slots, all 192 rows valid
            lengths = [len({pc[4] for pc in tail["pieces"] if pc[1] == i}) for i in range(len(tail["tiles"]))]
            assert max(lengths) >= 6, lengths        # pieces of many lengths in one tile
    elif name == "n_does_not_divide_the_tile":
        assert 192 // n == 27 and 27 * n == 189
        for t in images:
            tail = t[192]["tail"]
            assert tail["summary"]["full_tiles"] == 0          # even a tile that closes on its 27 slots leaves 3 padding rows
            ext = [x for x in tail["tiles"] if x[3] == "ext"]
            assert ext and all(192 - x[1] * n >= 3 + n for x in ext), tail["tiles"]        # closed on extended rows: many padding rows
    elif name == "edges":
        coarse0 = p - sum(w * h for w, h in levels[-2:])
        by = dict(zip(EDGE_CALLS, kept_calls))
        nothing = [not k.any() for k in by["nothing"]]
        assert any(nothing) and not all(nothing), "an image that keeps nothing beside images that keep something"
        assert any(k.any() and not k[:coarse0].any() for k in by["coarse"]), "an image whose kept pixels all lie in the two coarsest levels"
        assert any(k[0] for k in by["ends"]), "an image that keeps pixel 0"
        assert any(k[p - 1] for k in by["ends"]), "an image that keeps pixel P - 1"
    else:
        raise AssertionError(name)
    if name != "edges":                            # one engine, many masks: they differ between the images of a call and between calls
        assert len({k.tobytes() for k in masks}) == len(masks)


@pytest.mark.parametrize("name", list(CASES))
def test_sparse_plans_on_chosen_keep_sets(name):
    case = CASES[name]
    masks, stats = _run(case)
    kept_calls, replay_calls = [], []
    for i, device in enumerate(masks):
        kept, replay = _check_call(name, case, i, device, stats)
        kept_calls.append(kept)
        replay_calls.append(replay)
    _properties(name, case, kept_calls, replay_calls)
