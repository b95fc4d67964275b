"""Scratch, LDS and register budget of the five kernels of csrc/gsx_density.hip, from the compiler's own report (hipcc
cross-compiles: no GPU).  No scratch anywhere -- the apply kernel indexes its group descriptors inside the kernel-argument
segment with scalar loads instead of copying them to a private array, and its run table (2 KiB) and split offsets (6 KiB)
live in LDS; all five run at eight waves per SIMD.  These are the figures of the build tools/bench_densify.py timed at
0.570 ms for a round of the trained-like 1M scene, 0.303 ms of it the apply kernel (the table in DESIGN.md section 8b,
"Density control"): a change that moves one is to be re-measured."""
import os
import shutil

import pytest

from test_kernel_resources import HIPCC, _resources

# kernel -> (max VGPRs, LDS bytes per workgroup as declared, min waves per SIMD); scratch is 0 for all
BUDGET = {
    "density_accumulate_kernel": (13, 0, 8),
    "density_classify_kernel": (15, 1024, 8),
    "density_blocks_kernel": (22, 1024, 8),
    "density_final_kernel": (11, 1024, 8),
    "density_apply_kernel": (30, 8200, 8),       # table 2048 + offsets 6144 + the run's span 8
}

needs_tools = pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("c++filt") is None, reason="needs hipcc and c++filt")


@needs_tools
def test_density_kernels_use_no_scratch():
    table = _resources("gsx_density.hip")
    assert sorted(table) == sorted(BUDGET), sorted(table)
    for kernel, r in table.items():
        print(kernel, r)
        assert r["ScratchSize"] == 0, (kernel, r)


@needs_tools
@pytest.mark.parametrize("kernel", sorted(BUDGET))
def test_density_kernels_stay_inside_their_measured_budget(kernel):
    vgprs, lds, occupancy = BUDGET[kernel]
    r = _resources("gsx_density.hip")[kernel]
    assert r["VGPRs"] <= vgprs and r["LDS"] == lds and r["Occupancy"] >= occupancy, (kernel, r)
