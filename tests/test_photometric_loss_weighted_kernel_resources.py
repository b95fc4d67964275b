"""Scratch, LDS and register budget of the kernels of gsx_photometric_loss_weighted (csrc/gsx_loss_weighted.hip), from the
compiler's own report (hipcc cross-compiles: no GPU).  No scratch anywhere; LDS per workgroup at most 80 KiB of the CU's
160 KiB, so that two workgroups of wloss_maps_kernel share a CU as two of loss_maps_kernel do: the weight sits in registers
and the exposure is applied in place, so the LDS figures are those of gsx_loss.hip.  The VGPR counts are what this tree
compiles to -- a change that moves one is to be re-measured (tools/bench_loss.py --weighted).  Template arguments:
wloss_maps_kernel<with gradient, with exposure>, wloss_grad_kernel<with exposure>."""
import os
import shutil

import pytest

from test_kernel_resources import HIPCC, _resources

# kernel -> (max VGPRs, LDS bytes per workgroup as declared, min waves per SIMD); scratch is 0 for all of them
BUDGET = {
    "wloss_maps_kernel<true, true>": (82, 69216, 4),       # LDS admits two workgroups of eight waves: 4 per SIMD
    "wloss_maps_kernel<true, false>": (82, 69216, 4),
    "wloss_maps_kernel<false, true>": (71, 69216, 4),
    "wloss_maps_kernel<false, false>": (71, 69216, 4),
    "wloss_reduce_kernel": (22, 6144, 8),
    "wloss_grad_kernel<true>": (86, 37296, 5),
    "wloss_grad_kernel<false>": (82, 37296, 5),
    "wloss_exposure_reduce_kernel": (54, 24576, 6),        # one workgroup per call: twelve double sums side by side
    "wloss_weight_sum_kernel": (2, 0, 8),
}
LDS_LIMIT = 80 * 1024

needs_tools = pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("c++filt") is None, reason="needs hipcc and c++filt")


@needs_tools
def test_weighted_loss_kernels_use_no_scratch_and_leave_room_for_two_workgroups_per_cu():
    table = _resources("gsx_loss_weighted.hip")
    assert sorted(table) == sorted(BUDGET), sorted(table)
    for kernel, r in table.items():
        print(kernel, r)
        assert r["ScratchSize"] == 0, (kernel, r)
        assert r["LDS"] <= LDS_LIMIT, (kernel, r)


@needs_tools
@pytest.mark.parametrize("kernel", sorted(BUDGET))
def test_weighted_loss_kernels_stay_inside_their_measured_budget(kernel):
    vgprs, lds, occupancy = BUDGET[kernel]
    r = _resources("gsx_loss_weighted.hip")[kernel]
    assert r["VGPRs"] <= vgprs and r["LDS"] == lds and r["Occupancy"] >= occupancy, (kernel, r)
