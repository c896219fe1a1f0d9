"""GPU: ResNet stage 3 on the pointwise kernel's 512-channel tile (conv_pointwise.hip, pw_conv512_next_kernel): a block's 1x1
expansion `2c` (128 -> 512 + shortcut + ReLU) carries the NEXT block's 1x1 reduction `2a` (512 -> 128 + ReLU), computed from the
finished tile in LDS with one fp32 accumulator chain over all 32 k-steps (the second K half continues the first's accumulator).
BOD_PW_FUSE_NEXT3=0 plans the separate launches: nothing downstream may differ by one bit, and the fused plan is exactly three
launches shorter (stage 3 has four blocks in ResNet-50 and -101).  The stage-3 map is H/8 x W/8, tiles are 32 pixels:
one partial tile (64 px), a pixel count that is no multiple of 32 (720 px), several tiles per persistent workgroup with a ragged
last one, ResNet-101, and the full pipeline."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CODE = ("import numpy as np, sys; sys.path.insert(0, %r)\n"
        "from bayes_od_rc_amd import synthetic\n"
        "from bayes_od_rc_amd.anchor_generator import FpnAnchorGenerator\n"
        "from bayes_od_rc_amd.engine import Engine, make_config\n"
        "out = {}\n"
        "for tag, hw, b, depth in (('a', (64, 64), 1, 50), ('b', (96, 160), 3, 50), ('c', (192, 624), 2, 50), ('d', (128, 128), 2, 101)):\n"
        "    eng = Engine(make_config(hw, batch=b, mc_samples=2, backbone_depth=depth))\n"
        "    eng.load_weights(synthetic.make_weights(depth=depth))\n"
        "    eng.forward(synthetic.make_frames(b, hw[0], hw[1], seed=3), seed=11, first_image_id=2)\n"
        "    for l in range(5): out['%%s_p%%d' %% (tag, l)] = eng.get_pyramid(l)\n"
        "    for k, v in zip('cbv', eng.get_raw()): out['%%s_%%s' %% (tag, k)] = v\n"
        "    out[tag + '_ops'] = np.int32(eng.plan_info()['ops'])\n"
        "    eng.close()\n"
        "hw, b, n = (128, 128), 3, 3\n"
        "acfg = {'layers': [3, 4, 5, 6, 7], 'aspect_ratios': [[1.0, 1.0], [1.0, 2.0], [2.0, 1.0]], 'scales': [1.0, 1.26, 1.59]}\n"
        "eng = Engine(make_config(hw, batch=b, mc_samples=n))\n"
        "eng.load_weights(synthetic.make_weights(cls_fg_bias=-1.0))\n"
        "eng.set_anchors(FpnAnchorGenerator(acfg).generate_all((hw[0], hw[1], 3)))\n"
        "eng.infer(synthetic.make_frames(b, hw[0], hw[1], seed=1), seed=2024, first_image_id=0)\n"
        "for i in range(b):\n"
        "    for k, v in zip(('scores', 'means', 'covs', 'counts'), eng.get_detections(i)): out['det%%d_%%s' %% (i, k)] = np.asarray(v)\n"
        "eng.close()\n"
        "np.savez(sys.argv[1], **out)\n" % ROOT)


def _run(**switches):
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "o.npz")
        env = dict(os.environ, BOD_POINTWISE="1", BOD_POINTWISE_MIN_M="1", BOD_CHAIN_FUSION="0", BOD_CONV_SPLITK="0", **switches)
        r = subprocess.run([sys.executable, "-c", CODE, path], env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        z = np.load(path)
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def fused():
    return _run(BOD_PW_FUSE_NEXT3="1")


@pytest.fixture(scope="module")
def separate():
    return _run(BOD_PW_FUSE_NEXT3="0")


def _assert_same(got, want, prefixes):
    keys = [k for k in sorted(want) if k.startswith(prefixes) and not k.endswith("_ops")]
    assert keys and set(got) == set(want)
    for k in keys:
        assert got[k].shape == want[k].shape, k
        assert np.isfinite(got[k]).all() and np.isfinite(want[k]).all(), k
        assert np.array_equal(got[k], want[k]), (k, float(np.abs(got[k].astype(np.float64) - want[k]).max()))


@pytest.mark.parametrize("tag", ["a", "b", "c", "d"])
def test_stage3_fused_next_reduction_is_bit_identical(fused, separate, tag):
    """Every pyramid level and the raw head outputs, per shape; the plan is exactly three launches shorter."""
    _assert_same(fused, separate, (tag + "_",))
    assert len([k for k in fused if k.startswith(tag + "_")]) == 9
    assert np.abs(separate[tag + "_p0"]).max() > 0
    assert int(fused[tag + "_ops"]) == int(separate[tag + "_ops"]) - 3, (tag, int(fused[tag + "_ops"]), int(separate[tag + "_ops"]))


def test_stage3_fused_full_pipeline_detections_are_bit_identical(fused, separate):
    """infer at (128, 128), batch 3, N = 3: scores, means, covariances and counts of every image's detections."""
    _assert_same(fused, separate, ("det",))
    assert sum(int(separate["det%d_scores" % i].shape[0]) for i in range(3)) > 0


def test_stage3_switch_is_independent_of_stage2_switch(fused, separate):
    """BOD_PW_FUSE_NEXT=0 with BOD_PW_FUSE_NEXT3=1: stage 2's two fused launches are planned apart, stage 3's three stay fused."""
    mixed = _run(BOD_PW_FUSE_NEXT="0", BOD_PW_FUSE_NEXT3="1")
    _assert_same(mixed, separate, ("a_", "b_", "c_", "d_", "det"))
    for tag in "abcd":
        assert int(mixed[tag + "_ops"]) == int(fused[tag + "_ops"]) + 2 == int(separate[tag + "_ops"]) - 1, tag
