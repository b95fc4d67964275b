"""Scratch, LDS and register budget of the kernel of csrc/gsx_rectify.hip, from the compiler's own report (hipcc
cross-compiles: no GPU).  No scratch, no LDS -- the photo is gathered straight from global memory -- and eight waves per
SIMD.  These are the figures of the build tools/bench_rectify.py timed (the table in DESIGN.md section 8b, "Real captures"):
a change that moves one is to be re-measured."""
import os
import shutil

import pytest

from test_kernel_resources import HIPCC, _resources

# kernel -> (max VGPRs, LDS bytes per workgroup, min waves per SIMD)
BUDGET = {"rectify_kernel": (45, 0, 8)}

needs_tools = pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("c++filt") is None, reason="needs hipcc and c++filt")


@needs_tools
def test_rectify_kernel_uses_no_scratch_and_stays_inside_its_measured_budget():
    table = _resources("gsx_rectify.hip")
    assert sorted(table) == sorted(BUDGET), sorted(table)
    for kernel, (vgprs, lds, occupancy) in BUDGET.items():
        r = table[kernel]
        print(kernel, r)
        assert r["ScratchSize"] == 0, (kernel, r)
        assert r["VGPRs"] <= vgprs and r["LDS"] == lds and r["Occupancy"] >= occupancy, (kernel, r)
