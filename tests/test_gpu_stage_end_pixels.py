"""GPU: the last block of ResNet stages 2-4 on the pixels that are read (engine.hip build_plan, plane_tables.h).  The output of res2c,
res3d and res4f (res4w in ResNet-101) has one reader, the next stage's 1x1 stride-2 VALID `2a` / `branch1`: the block's `2c` runs on
the table of output pixels (2y, 2x), stage 4's `2b` on the even rows of its row-reuse tiles.  BOD_STAGE_END_PIXELS=0 plans the whole
planes: the handle's device bytes are the same (the step-2 tables live in the dense tables' entries), all five pyramid levels, the
raw head outputs and the detections may not differ by one bit, the op count stays, the three
`2c` ops have M = B * ceil(h / 2) * ceil(w / 2) (BOD_DUMP_OPS), a training handle keeps the whole planes.  Geometries 64x64, 96x160 and
104x75 (stage planes 15x15 / 8x8 / 4x4, 23x40 / 12x20 / 6x10 and 25x19 / 13x10 / 7x5: odd in both directions at several stages, so
ceil(. / 2) and the last row and column are exercised; a 100x75 image is refused by bod_create -- its p3 plane is 12 rows against an
anchor grid of 13 -- and 104x75 is the size with the 25x19, 13x10 and 7x5 planes), batch 1 and 3, N = 2; once on the planner's own choice
of kernels, once with the streaming kernels forced at these sizes (BOD_POINTWISE_MIN_M=1: the pointwise and sliding-window
floors) and once with the 256x256 tiles forced, where stage 4's `2b` runs on row-reuse tiles; ResNet-101 and every precision once."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GEOMETRIES = ((64, 64), (96, 160), (104, 75))
# (tag, image size, batch, depth, precision): in the order the child builds its handles (the BOD_DUMP_OPS blocks follow it)
CASES = tuple(("g%dx%d_b%d" % (hw[0], hw[1], b), hw, b, 50, "bf16") for hw in GEOMETRIES for b in (1, 3)) + \
        (("r101", (96, 160), 3, 101, "bf16"),) + \
        tuple(("p_" + p, (104, 75), 3, 50, p) for p in ("fp32", "bf16x3", "f16mx", "f16mx4"))

CODE = ("import numpy as np, sys; sys.path.insert(0, %r)\n"
        "from bayes_od_rc_amd import synthetic\n"
        "from bayes_od_rc_amd.anchor_generator import FpnAnchorGenerator\n"
        "from bayes_od_rc_amd.engine import Engine, make_config\n"
        "acfg = {'layers': [3, 4, 5, 6, 7], 'aspect_ratios': [[1.0, 1.0], [1.0, 2.0], [2.0, 1.0]], 'scales': [1.0, 1.26, 1.59]}\n"
        "out, weights = {}, {}\n"
        "for tag, hw, b, depth, prec in %r:\n"
        "    if depth not in weights: weights[depth] = synthetic.make_weights(depth=depth, cls_fg_bias=-1.0)\n"
        "    eng = Engine(make_config(hw, batch=b, mc_samples=2, backbone_depth=depth, precision=prec))\n"
        "    eng.load_weights(weights[depth])\n"
        "    eng.set_anchors(FpnAnchorGenerator(acfg).generate_all((hw[0], hw[1], 3)))\n"
        "    frames = synthetic.make_frames(b, hw[0], hw[1], seed=3)\n"
        "    eng.forward(frames, seed=11, first_image_id=2)\n"
        "    for l in range(5): out['%%s_p%%d' %% (tag, l)] = eng.get_pyramid(l)\n"
        "    for k, v in zip('cbv', eng.get_raw()): out['%%s_%%s' %% (tag, k)] = v\n"
        "    eng.infer(frames, seed=2024, first_image_id=0)\n"
        "    for i in range(b):\n"
        "        for k, v in zip(('scores', 'means', 'covs', 'counts'), eng.get_detections(i)): out['%%s_det%%d_%%s' %% (tag, i, k)] = np.asarray(v)\n"
        "    info = eng.plan_info()\n"
        "    out[tag + '_ops'] = np.int32(info['ops'])\n"
        "    out[tag + '_slot'] = np.int32(info['stage_end_pixels'])\n"
        "    out[tag + '_xr'] = np.int32(info['plane_row_reuse_layers'])\n"
        "    out[tag + '_bytes'] = np.int64(eng.device_bytes)\n"
        "    eng.close()\n"
        "eng = Engine(make_config((64, 64), batch=2, mc_samples=1, training=True))\n"
        "eng.load_weights(weights[50])\n"
        "out['train_slot'] = np.int32(eng.plan_info()['stage_end_pixels'])\n"
        "eng.close()\n"
        "np.savez(sys.argv[1], **out)\n" % (ROOT, CASES))


def _run(**switches):
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "o.npz")
        env = dict(os.environ, BOD_DUMP_OPS="1", **switches)
        r = subprocess.run([sys.executable, "-c", CODE, path], env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        z = np.load(path)
        res = {k: z[k] for k in z.files}
        # one block of '# op' lines per handle, in CASES' order (the training handle's comes last)
        blocks = [b for b in r.stderr.split("# ops:")[1:]]
        assert len(blocks) == len(CASES) + 1, len(blocks)
        res["dump"] = [dict((m.group(2), int(m.group(3))) for m in re.finditer(r"^# op (\d+) (\S+) \d+ -?\d+ (\d+) ", b, flags=re.M)) for b in blocks]
        return res


@pytest.fixture(scope="module")
def runs():
    forced = dict(BOD_POINTWISE="1", BOD_POINTWISE_MIN_M="1")
    # (the 256x256 tiles at these sizes, no split-K: stage 4's `2b` layers run on the row-reuse tiles, the last on its even rows)
    tiles = dict(BOD_FORCE_CONV_TILE="256", BOD_CONV_SPLITK="0")
    return {("own", 1): _run(), ("own", 0): _run(BOD_STAGE_END_PIXELS="0"),
            ("forced", 1): _run(**forced), ("forced", 0): _run(BOD_STAGE_END_PIXELS="0", **forced),
            ("tiles", 1): _run(**tiles), ("tiles", 0): _run(BOD_STAGE_END_PIXELS="0", **tiles)}


def _assert_same(got, want, prefix):
    keys = [k for k in sorted(want) if k.startswith(prefix) and not k.endswith(("_ops", "_slot", "_xr", "_bytes"))]
    assert keys and set(got) == set(want)
    for k in keys:
        assert got[k].shape == want[k].shape, k
        assert np.isfinite(got[k]).all() and np.isfinite(want[k]).all(), k
        assert np.array_equal(got[k], want[k]), (k, float(np.abs(got[k].astype(np.float64) - want[k]).max()))
    return keys


def _stage_planes(hw):
    cdiv = lambda a, b: (a + b - 1) // b
    sh, sw = (hw[0] - 7) // 2 + 1, (hw[1] - 7) // 2 + 1          # stem (7x7, stride 2) and pool (3x3, stride 2): build_geometry
    h, w = (sh + 2 - 3) // 2 + 1, (sw + 4 - 3) // 2 + 1
    planes = {}
    for st in (2, 3, 4):
        planes[st] = (h, w)
        h, w = cdiv(h, 2), cdiv(w, 2)
    return planes


@pytest.mark.parametrize("kernels", ["own", "forced", "tiles"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_stage_end_pixels_is_bit_identical(runs, kernels, case):
    """Pyramid levels, raw head outputs and detections with the switch on and off; slot 10 and the op count."""
    tag, hw, b = case[0], case[1], case[2]
    on, off = runs[(kernels, 1)], runs[(kernels, 0)]
    keys = _assert_same(on, off, tag + "_")
    assert len(keys) == 8 + 4 * b
    assert np.abs(off[tag + "_p0"]).max() > 0 and np.abs(off[tag + "_c"]).max() > 0
    assert int(on[tag + "_slot"]) == 2 and int(off[tag + "_slot"]) == 0
    assert int(on[tag + "_ops"]) == int(off[tag + "_ops"])
    assert int(on[tag + "_xr"]) == int(off[tag + "_xr"])
    if kernels != "tiles":          # the step-2 tables live in the dense tables: no byte more (the even-row tiling has tables of its own)
        assert int(on[tag + "_bytes"]) == int(off[tag + "_bytes"])
    if kernels == "tiles" and case[4] != "fp32":          # every `2b` of stage 4 and P3-P5 of the FPN: the last block's is among them
        assert int(on[tag + "_xr"]) == (23 if case[3] == 101 else 6) + 3


@pytest.mark.parametrize("kernels", ["own", "forced"])
def test_detections_exist(runs, kernels):
    off = runs[(kernels, 0)]
    assert sum(int(off[k].shape[0]) for k in off if k.endswith("_scores")) > 0


@pytest.mark.parametrize("kernels", ["own", "forced"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_last_2c_ops_run_on_a_quarter_of_the_rows(runs, kernels, case):
    """BOD_DUMP_OPS: M of res2c / res3d / res4f (res4w) _branch2c is B * ceil(h / 2) * ceil(w / 2); the other ops keep their M."""
    _, hw, b, depth, _ = case
    i = CASES.index(case)
    on, off = runs[(kernels, 1)]["dump"][i], runs[(kernels, 0)]["dump"][i]
    assert list(on) == list(off)
    planes = _stage_planes(hw)
    last = {2: "res2c_branch2c", 3: "res3d_branch2c", 4: "res4w_branch2c" if depth == 101 else "res4f_branch2c"}
    for st, name in last.items():
        h, w = planes[st]
        assert off[name] == b * h * w, (name, off[name])
        assert on[name] == b * ((h + 1) // 2) * ((w + 1) // 2), (name, on[name], h, w)
    changed = set(last.values()) | {last[4].replace("2c", "2b")}          # (stage 4's 2b: even rows when it runs on row-reuse tiles)
    for name in off:
        if name not in changed:
            assert on[name] == off[name], name
    assert on[last[4].replace("2c", "2b")] <= off[last[4].replace("2c", "2b")]


def test_training_handle_keeps_whole_planes(runs):
    for r in runs.values():
        assert int(r["train_slot"]) == 0
    train_on, train_off = runs[("own", 1)]["dump"][-1], runs[("own", 0)]["dump"][-1]
    assert train_on == train_off and "res2c_branch2c" in train_on
