"""Scratch, LDS and register budget of the three kernels of gsx_photometric_loss (csrc/gsx_loss.hip), from the compiler's
own report (hipcc cross-compiles: no GPU).  No scratch anywhere; LDS per workgroup at most 80 KiB of the CU's 160 KiB, so
that two workgroups of loss_maps_kernel (the tile + halo of both images in three channel planes + five row-filtered planes)
share a CU; the VGPR counts are the ones the tree was measured with -- a change that moves one is to be re-measured
(tools/bench_loss.py)."""
import os
import shutil

import pytest

from test_kernel_resources import HIPCC, _resources

# kernel -> (max VGPRs, LDS bytes per workgroup as declared, min waves per SIMD); scratch is 0 for all of them
BUDGET = {
    "loss_maps_kernel<true>": (100, 69216, 4),       # LDS admits two workgroups of eight waves: 4 per SIMD whatever the registers
    "loss_maps_kernel<false>": (69, 69216, 4),
    "loss_reduce_kernel": (17, 4096, 8),
    "loss_grad_kernel": (81, 37296, 5),
}
LDS_LIMIT = 80 * 1024

needs_tools = pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("c++filt") is None, reason="needs hipcc and c++filt")


@needs_tools
def test_loss_kernels_use_no_scratch_and_leave_room_for_two_workgroups_per_cu():
    table = _resources("gsx_loss.hip")
    assert sorted(table) == sorted(BUDGET), sorted(table)
    for kernel, r in table.items():
        print(kernel, r)
        assert r["ScratchSize"] == 0, (kernel, r)
        assert r["LDS"] <= LDS_LIMIT, (kernel, r)


@needs_tools
@pytest.mark.parametrize("kernel", sorted(BUDGET))
def test_loss_kernels_stay_inside_their_measured_budget(kernel):
    vgprs, lds, occupancy = BUDGET[kernel]
    r = _resources("gsx_loss.hip")[kernel]
    assert r["VGPRs"] <= vgprs and r["LDS"] == lds and r["Occupancy"] >= occupancy, (kernel, r)
