"""Registers of project_x3_claim_kernel (csrc/project.h), the streaming projection's form that runs beside the hop launches: it is built for
four waves per SIMD (128 VGPRs) so that one of its waves displaces two hop waves and not more, and it must stay as spill-free as the 1024-thread
form is held to in test_host_logic.py::test_hot_kernels_do_not_spill.  Today five of the six instantiations have no scratch at all; <4, 2> (rows of
64 floats, 64 columns: the headline's) parks ONE 64-bit address (2 VGPRs, 12 bytes), stored once in front of the tile loop and loaded once per
16-row tile, outside the unit loop that does the tile's work.  Read from the built library's own metadata (tools/kernel_resources.py)."""
import os

import pytest


def test_claim_kernel_registers_and_scratch():
    from tgcn_amd import _lib
    from tools import kernel_resources as kr
    if not os.path.exists(_lib.LIB_PATH) or not os.path.exists(os.path.join(kr.LLVM, "llvm-readelf")):
        pytest.skip("needs the built library and llvm-readelf")
    res = kr.kernel_resources(_lib.LIB_PATH)
    claim = {k: v for k, v in res.items() if "23project_x3_claim_kernel" in k}
    assert len(claim) == 6, sorted(claim)
    for name, r in claim.items():
        assert r["max_flat_workgroup_size"] == 256, (name, r)
        assert r["vgpr_count"] + r["agpr_count"] <= 128, (name, r)                   # four waves per SIMD
        assert r["group_segment_fixed_size"] == 0, (name, r)                         # LDS: the weight planes only (dynamic)
        assert r["sgpr_spill_count"] == 0 and r["uses_dynamic_stack"] in ("false", 0), (name, r)
        if "ILi4ELi2E" in name:
            assert r["vgpr_spill_count"] <= 2 and r["private_segment_fixed_size"] <= 12, (name, r)
        else:
            assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (name, r)
