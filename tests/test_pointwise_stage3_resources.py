"""CPU (hipcc cross-compile): resources of stage 3's fused pointwise kernel (conv_pointwise.hip, pw_conv512_next_kernel: the 1x1
expansion 128 -> 512 that carries the next block's 1x1 reduction 512 -> 128).  Its LDS-DMA waits are hand-counted
`s_waitcnt vmcnt(n)`: a scratch access would be a vector-memory instruction the counts do not know, so zero scratch is part of
the kernel's correctness, not only of its speed."""
import os
import shutil
import subprocess

import pytest

from bayes_od_rc_amd import build as build_mod
from bayes_od_rc_amd import kernel_guard as guard

KERNEL = "pw_conv512_next_kernel"


@pytest.fixture(scope="module")
def pointwise_meta(tmp_path_factory):
    """conv_pointwise.hip compiled on its own with build.py's flags -> the code object's kernel metadata."""
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("pw3")
    obj = str(d / "conv_pointwise.o")
    extra = dict(build_mod.SOURCES)["conv_pointwise.hip"]
    subprocess.check_call([build_mod._hipcc()] + build_mod.COMMON + extra + ["-c", os.path.join(build_mod.CSRC, "conv_pointwise.hip"), "-o", obj])
    return obj, guard.kernel_metadata(guard.extract_device_object(obj, str(d)))


def test_stage3_fused_kernel_uses_no_scratch(pointwise_meta):
    obj, meta = pointwise_meta
    hits = {n: f for n, f in meta.items() if KERNEL in n}
    assert len(hits) == 1, sorted(meta)
    guard.check_no_spills(meta, wanted=[KERNEL])
    for n, f in hits.items():
        assert f.get("private_segment_fixed_size", 0) == 0 and f.get("vgpr_spill_count", 0) == 0 and f.get("sgpr_spill_count", 0) == 0, (n, f)
        # eight waves, one workgroup per CU: two waves per SIMD share its 512 registers per lane
        assert f["vgpr_count"] + f.get("agpr_count", 0) <= 256, (n, f)
    regs = guard.verify_pointwise_stage3(obj)
    assert len(regs) == 1 and all(v <= 256 for v in regs.values()), regs


def test_sparse_tower_kernel_keeps_its_resources_with_the_xcd_tile_order(tmp_path):
    """The sparse launches' XCD-contiguous tile order lives in conv_igemm_kernel's wrapper (the `tile_count` branch): the tower kernel
    must stay where tests/test_kernel_resources.py pins it -- no spill, no scratch, at most the 256 registers of two waves per SIMD --
    and its hand-counted LDS waits must still replay."""
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    build_mod.build(verbose=False)                   # no-op when the tree is built
    tower = "conv_igemm_kernelILi256ELi256ELi2ELi4ELi0ELb1ELb0EE"
    assert tower in guard.PRODUCTION and tower in guard.INLINE_ASM_LDS
    co = guard.extract_device_object(os.path.join(build_mod.LIB_DIR, "obj", "conv_igemm.o"), str(tmp_path))
    meta = guard.kernel_metadata(co)
    guard.check_no_spills(meta, wanted=[tower])
    hits = {n: f for n, f in meta.items() if tower in n}
    assert len(hits) == 1, sorted(hits)
    for n, f in hits.items():
        assert f.get("private_segment_fixed_size", 0) == 0 and f.get("vgpr_spill_count", 0) == 0, (n, f)
        assert f["vgpr_count"] + f.get("agpr_count", 0) <= 256, (n, f)
    funcs = guard.disassemble(co, with_addr=True)
    assert sum(guard.check_asm_lds_reads(funcs[n], tower) for n in funcs if tower in n) >= 6 + 2 * 72


def test_the_build_guards_the_stage3_kernel():
    """build.build() refuses to link a library whose stage-3 kernel spills (kernel_guard.verify_pointwise_stage3 on the object
    about to be linked); the streaming kernels' own guard list is unchanged."""
    assert guard.POINTWISE_STAGE3 == [KERNEL] and KERNEL not in guard.POINTWISE_PRODUCTION
    with pytest.raises(guard.GuardError, match="spills"):
        guard.check_no_spills({"_Z22" + KERNEL + "8ConvArgsii": {"vgpr_spill_count": 6, "private_segment_fixed_size": 28}}, wanted=[KERNEL])
