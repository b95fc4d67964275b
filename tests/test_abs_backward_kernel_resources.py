"""Register, scratch and LDS budget of the backward compositing kernel's abs instance (gsx_render_backward_screen_abs), from the
compiler's own report (tests/test_kernel_resources.py's helpers; hipcc cross-compiles: no GPU).  It is the geometry instance
with two more accumulators per record and three hoisted conic sums: it may not use scratch, and it is held to the geometry
instance's 4 waves per SIMD (a budget of 128 VGPRs), which the compiler gives it at 116.  The three older instances beside
it keep the registers, occupancy and LDS they had; the per-Gaussian sum's abs instance beside them stays small."""
import os
import shutil

import pytest

from test_kernel_resources import HIPCC, _resources

ABS_TILE_VGPRS = 116        # backward_tile_abs_kernel as the compiler reports it (the geometry instance: 108)
ABS_TILE_WAVES = 4
ABS_TILE_LDS = 3 * 64 * 16 + 64 * 4 + 64 * 4 * 4 + 64 * 7 * 4     # three staged float4 arrays, slots, four colour sums, seven geometry sums


@pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("c++filt") is None, reason="needs hipcc and c++filt")
def test_the_abs_instance_keeps_the_geometry_instance_s_occupancy_and_moves_no_other():
    table = _resources("gsx_backward.hip")
    tile = table["backward_tile_abs_kernel"]
    print("abs", tile, "sum", table["backward_geometry_abs_sum_kernel"])
    assert tile["ScratchSize"] == 0, tile
    assert tile["VGPRs"] <= ABS_TILE_VGPRS and tile["Occupancy"] >= ABS_TILE_WAVES, tile
    assert tile["LDS"] == ABS_TILE_LDS, tile
    small = table["backward_geometry_abs_sum_kernel"]
    assert small["ScratchSize"] == 0 and small["VGPRs"] <= 32 and small["LDS"] == 0, small
    # the instances the older entries run, as the merged tests hold them
    colour, geometry, depth = (table[k] for k in ("backward_tile_kernel", "backward_tile_geometry_kernel", "backward_tile_depth_kernel"))
    assert colour["VGPRs"] <= 128 and colour["ScratchSize"] == 0 and colour["LDS"] == 4352, colour
    assert geometry["VGPRs"] <= 108 and geometry["ScratchSize"] == 0 and geometry["Occupancy"] >= 4 and geometry["LDS"] == 5632, geometry
    assert depth["VGPRs"] <= 180 and depth["ScratchSize"] == 0 and depth["Occupancy"] >= 2 and depth["LDS"] == 6144, depth
    for kernel in ("backward_geometry_sum_kernel", "backward_geometry_chain_kernel"):
        assert table[kernel]["ScratchSize"] == 0, (kernel, table[kernel])
