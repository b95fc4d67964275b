"""Scratch, LDS and register budget of the kernels the screen-space statistic adds or touches, from the compiler's own report
(hipcc cross-compiles: no GPU).  csrc/gsx_density_screen.hip holds exactly its two kernels, both free of scratch and at eight
waves per SIMD: the figures of the build tools/bench_densify.py --screen timed ("Screen-space
statistic").  The chain kernel that now also delivers dL/d(NDC mean) and the radius stays free of scratch at the four waves
per SIMD it had, and project_raw_kernel, which now keeps the radius it used to drop, stays at eight."""
import os
import shutil

import pytest

from test_kernel_resources import HIPCC, _resources

# kernel -> (max VGPRs, LDS bytes per workgroup as declared, min waves per SIMD); scratch is 0 for all
BUDGET = {
    "density_accumulate_screen_kernel": (13, 0, 8),
    "density_classify_screen_kernel": (16, 1024, 8),
}

needs_tools = pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("c++filt") is None, reason="needs hipcc and c++filt")


@needs_tools
def test_the_screen_density_file_holds_its_two_kernels_without_scratch():
    table = _resources("gsx_density_screen.hip")
    assert sorted(table) == sorted(BUDGET), sorted(table)
    for kernel, r in table.items():
        print(kernel, r)
        vgprs, lds, occupancy = BUDGET[kernel]
        assert r["ScratchSize"] == 0, (kernel, r)
        assert r["VGPRs"] <= vgprs and r["LDS"] == lds and r["Occupancy"] >= occupancy, (kernel, r)


@needs_tools
def test_the_chain_and_raw_projection_kernels_keep_their_occupancy():
    chain = _resources("gsx_backward.hip")["backward_geometry_chain_kernel"]
    raw = _resources("gsx_project.hip")["project_raw_kernel"]
    print("chain", chain, "raw", raw)
    assert chain["ScratchSize"] == 0 and chain["Occupancy"] >= 4 and chain["VGPRs"] <= 128, chain
    assert raw["ScratchSize"] == 0 and raw["Occupancy"] >= 8, raw
