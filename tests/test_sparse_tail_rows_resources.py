"""CPU (hipcc cross-compile): resources of the sparse tail's tower kernel on 192-row tiles, conv_igemm_kernel<256, 192, 2, 4, 0, true>
(conv_igemm.hip: the row-reuse loop with three 16-row pixel fragments per wave).  Like the 256-row symbol it runs one workgroup of
eight waves per compute unit -- two waves per SIMD, so at most 256 registers per lane, no spill and no scratch (a scratch access is
a vector-memory instruction the loop's hand-counted vmcnt waits do not know) -- inside the 160 KiB of LDS, and its loop issues three
MFMAs per step where the 256-row loop issues four."""
import os
import re
import shutil

import pytest

from bayes_od_rc_amd import build as build_mod
from bayes_od_rc_amd import kernel_guard as guard

TAIL192 = "conv_igemm_kernelILi256ELi192ELi2ELi4ELi0ELb1ELb0EE"
TOWER256 = "conv_igemm_kernelILi256ELi256ELi2ELi4ELi0ELb1ELb0EE"


@pytest.fixture(scope="module")
def conv_code_object(tmp_path_factory):
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    build_mod.build(verbose=False)                   # no-op when the tree is built
    return guard.extract_device_object(os.path.join(build_mod.LIB_DIR, "obj", "conv_igemm.o"), str(tmp_path_factory.mktemp("tail192")))


def test_the_192_row_symbol_is_guarded_by_the_build():
    assert guard.PRODUCTION[-1] == TAIL192                       # appended: other tests index the list from the front
    assert TAIL192 in guard.INLINE_ASM_MFMA and TAIL192 in guard.INLINE_ASM_LDS
    assert TOWER256 in guard.INLINE_ASM_MFMA and TOWER256 in guard.INLINE_ASM_LDS
    assert guard.MIN_LOOP_MFMA[TAIL192] * 4 == guard.MIN_LOOP_MFMA[TOWER256] * 3


def test_no_spill_no_scratch_two_waves_per_simd(conv_code_object):
    meta = guard.kernel_metadata(conv_code_object)
    guard.check_no_spills(meta, wanted=[TAIL192])
    hits = {n: f for n, f in meta.items() if TAIL192 in n}
    assert len(hits) == 1, sorted(hits)
    for n, f in hits.items():
        assert f.get("private_segment_fixed_size", 0) == 0 and f.get("vgpr_spill_count", 0) == 0 and f.get("sgpr_spill_count", 0) == 0, (n, f)
        assert f["vgpr_count"] + f.get("agpr_count", 0) <= 256, (n, f)
        print(n, f)


def test_lds_fits_the_compute_unit(conv_code_object):
    """The tile's LDS is dynamic (ConvCfg<256, 192, 2, 4, true>::LDS, which launch_cfg asserts at compile time): the same sum here,
    from the header's constants, plus whatever the code object declares statically.  The guard proper is that static_assert in
    launch_cfg, which sees the size the launch passes; this test restates ConvCfg's sum and would not follow a change of ConvCfg -- it
    pins that the assertion is there, that the code object adds no static LDS on top, and today's figure."""
    src = open(os.path.join(build_mod.CSRC, "conv_igemm.hip")).read()
    assert re.search(r"static_assert\(Cfg::LDS <= 160 \* 1024", src)
    ext_rows = int(re.search(r"constexpr int XR_EXT_ROWS = (\d+);", open(os.path.join(build_mod.CSRC, "plan_tables.h")).read()).group(1))
    bc, bp = 256, 192
    staged = 2 * bc * 128 + 2 * ext_rows * 128               # two weight stages + two extended-row buffers of 128-byte K-tile rows
    main = max(staged, bp * bc * 2)                          # ... or the bf16 output tile
    lds = main + bp * 4 + bp * 4 + bp * 8 + bc * 4 + bp * 4  # + output / residual pixels, dropout counters, bias, 1x1 output rows
    meta = guard.kernel_metadata(conv_code_object)
    static = [f.get("group_segment_fixed_size", 0) for n, f in meta.items() if TAIL192 in n]
    assert len(static) == 1
    assert lds + static[0] <= 160 * 1024, (lds, static)
    # the fused 1x1's fp32 output tile [192][cout2 rounded up to 32, + 4] reuses the staging area: the covariance head's 90 channels
    assert bp * (96 + 4) * 4 <= main


def test_loop_has_three_quarters_of_the_mfmas_and_replays(conv_code_object):
    funcs = guard.disassemble(conv_code_object)
    count = {}
    for want in (TAIL192, TOWER256):
        names = [n for n in funcs if want in n]
        assert len(names) == 1, (want, names)
        count[want] = guard.check_inline_asm_mfma(funcs[names[0]], want)
    assert count[TAIL192] * 4 == count[TOWER256] * 3, count
    funcs_a = guard.disassemble(conv_code_object, with_addr=True)
    walked = sum(guard.check_asm_lds_reads(funcs_a[n], TAIL192) for n in funcs_a if TAIL192 in n)
    # two trips over three unrolled K-tiles of 16 A + 2 x 3 B fragment reads, and the prologue's
    assert walked >= 5 + 2 * 66, walked


def test_wait_tables_in_the_source_are_the_replay_of_three_fragments():
    """The three-fragment `lgkmcnt` tables of conv_igemm.hip are what tests/tools/lds_wait_tables_frags.py derives, and that tool with
    four fragments is tests/tools/lds_wait_tables.py."""
    import importlib.util
    tools = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools")
    mods = []
    for name in ("lds_wait_tables_frags", "lds_wait_tables"):
        spec = importlib.util.spec_from_file_location(name, os.path.join(tools, name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mods.append(mod)
    frags, base = mods
    for ahead in (2, 3):
        for prev_last, last in ((False, False), (False, True), (True, False)):
            assert frags.sim(ahead, prev_last, last, 4) == base.sim(ahead, prev_last, last)
    src = open(os.path.join(build_mod.CSRC, "conv_igemm.hip")).read()
    for name, last in (("W_SAME2F3", False), ("W_LAST2F3", True)):
        m = re.search(r"constexpr int %s\[16\] = \{([^}]*)\};" % name, src)
        assert m, name
        assert [int(x) for x in m.group(1).split(",")] == frags.sim(2, False, last, 3), name
    # a group's first K-tile (the one before was a group's last): step 0 waits lgkmcnt(1), later steps take the smaller W_SAME counts
    first = frags.sim(2, True, False, 3)
    assert first[0] == 1 and all(a <= b for a, b in zip(frags.sim(2, False, False, 3)[1:14], first[1:14]))
