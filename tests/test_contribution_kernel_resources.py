"""Register and scratch budget of gsx_render_contribution's kernels, from the compiler's own report
(tests/test_kernel_resources.py's helpers; hipcc cross-compiles: no GPU).  The two tile kernels walk the lists the
colour-only backward instance walks and are held to its budget -- no scratch, at most 128 VGPRs -- and to four waves per
SIMD; they are two instances of one templated body, load no image and no gradient and carry one accumulator pair where that
instance carries fifteen floats per pixel, and what the compiler reports is recorded below."""
import os
import shutil

import pytest

from test_kernel_resources import HIPCC, _resources

COLOUR_ONLY_VGPRS = 128         # backward_tile_kernel's budget (tests/test_kernel_resources_depth.py)
MIN_WAVES = 4
# as measured on this tree
TILE_VGPRS = 48                 # contribution_tile_kernel, 8 waves per SIMD, 3072 B LDS
TILE_STD_VGPRS = 48             # contribution_tile_std_kernel, 8 waves per SIMD, 3072 B LDS
SUM_VGPRS = 17                  # contribution_sum_kernel, 8 waves per SIMD
PLAN_VGPRS = 12                 # density_classify_contribution_kernel


@pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("c++filt") is None, reason="needs hipcc and c++filt")
def test_contribution_kernels_keep_the_colour_only_budget():
    table = _resources("gsx_contribution.hip")
    names = ("contribution_tile_kernel", "contribution_tile_std_kernel", "contribution_sum_kernel")
    for kernel in names:
        assert kernel in table, (kernel, sorted(table))
    assert sorted(k for k in table if k.startswith("contribution_")) == sorted(names)       # the tile kernels are exactly two
    print({k: table[k] for k in names})
    for kernel, measured in zip(names, (TILE_VGPRS, TILE_STD_VGPRS, SUM_VGPRS)):
        row = table[kernel]
        assert row["ScratchSize"] == 0, (kernel, row)
        assert row["VGPRs"] <= COLOUR_ONLY_VGPRS and row["Occupancy"] >= MIN_WAVES, (kernel, row)
        assert row["VGPRs"] <= measured, (kernel, row)      # the recorded figure: a rise is a change someone should see
    plan = table["density_classify_contribution_kernel"]
    assert plan["ScratchSize"] == 0 and plan["VGPRs"] <= PLAN_VGPRS, plan
