"""Scratch, LDS and register budget of the two instances of gsx_adam_step's kernel (csrc/gsx_adam.hip), from the compiler's
own report (hipcc cross-compiles: no GPU).  No scratch -- the group descriptors are indexed inside the kernel-argument
segment with scalar loads, not copied to a private array; the skip instance's only LDS is its 256 row marks; both run at
eight waves per SIMD.  These are the figures of the build tools/bench_adam.py timed at 0.3275 ms dense / 0.3091 ms with the
skip on the trained-like 1M scene (the table in DESIGN.md section 8b, "Optimiser step"): a change that moves one is to be
re-measured."""
import os
import shutil

import pytest

from test_kernel_resources import HIPCC, _resources

# kernel -> (max VGPRs, LDS bytes per workgroup as declared, min waves per SIMD); scratch is 0 for both
BUDGET = {
    "adam_kernel<false>": (41, 0, 8),        # dense
    "adam_kernel<true>": (45, 1024, 8),      # GSX_ADAM_SKIP_ZERO_ROWS
}

needs_tools = pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("c++filt") is None, reason="needs hipcc and c++filt")


@needs_tools
def test_adam_kernels_use_no_scratch():
    table = _resources("gsx_adam.hip")
    assert sorted(table) == sorted(BUDGET), sorted(table)
    for kernel, r in table.items():
        print(kernel, r)
        assert r["ScratchSize"] == 0, (kernel, r)


@needs_tools
@pytest.mark.parametrize("kernel", sorted(BUDGET))
def test_adam_kernels_stay_inside_their_measured_budget(kernel):
    vgprs, lds, occupancy = BUDGET[kernel]
    r = _resources("gsx_adam.hip")[kernel]
    assert r["VGPRs"] <= vgprs and r["LDS"] == lds and r["Occupancy"] >= occupancy, (kernel, r)
