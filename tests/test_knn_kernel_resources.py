"""Scratch, LDS and register budget of the two kernels of csrc/gsx_knn.hip, from the compiler's own report (hipcc
cross-compiles: no GPU).  No scratch anywhere -- the three best squared distances, the query and the block fetched ahead
stay in registers; the staged block (4 KiB), the list of blocks to visit (1 KiB) and the per-wave partial results live in LDS;
both run at eight waves per SIMD.  These are the figures of the build tools/bench_knn.py timed (the table in DESIGN.md section
8b, "Scale initialisation"): a change that moves one is to be re-measured."""
import os
import shutil

import pytest

from test_kernel_resources import HIPCC, _resources

# kernel -> (max VGPRs, LDS bytes per workgroup as declared, min waves per SIMD); scratch is 0 for both
BUDGET = {
    "knn_gather_kernel": (28, 96, 8),           # the four waves' box corners: 4 x 6 floats
    "knn_search_kernel": (53, 5152, 8),         # tile 4096 + list 1024 + per-wave counts 16 + per-wave r3 16
}

needs_tools = pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("c++filt") is None, reason="needs hipcc and c++filt")


@needs_tools
def test_knn_kernels_use_no_scratch():
    table = _resources("gsx_knn.hip")
    assert sorted(table) == sorted(BUDGET), sorted(table)
    for kernel, r in table.items():
        print(kernel, r)
        assert r["ScratchSize"] == 0, (kernel, r)


@needs_tools
@pytest.mark.parametrize("kernel", sorted(BUDGET))
def test_knn_kernels_stay_inside_their_measured_budget(kernel):
    vgprs, lds, occupancy = BUDGET[kernel]
    r = _resources("gsx_knn.hip")[kernel]
    assert r["VGPRs"] <= vgprs and r["LDS"] == lds and r["Occupancy"] >= occupancy, (kernel, r)
