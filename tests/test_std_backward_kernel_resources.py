"""Register, scratch and LDS budget of the backward compositing kernel's two GSX_SEM_STD_3DGS instances
(gsx_render_backward_std), from the compiler's own report (tests/test_kernel_resources.py's helpers; hipcc cross-compiles:
no GPU).  The geometry instance is the ref_cpu geometry instance with another alpha, a clamp predicate and two skip rules:
it may not use scratch and is held to that instance's waves per SIMD, its LDS and -- since both are pinned to 4 waves, a
budget of 128 VGPRs -- to no more registers than the occupancy allows.  The numbers it is compared with are read from the
SAME build, not recorded here.  The four older instances keep what the merged tests hold them to."""
import os
import shutil

import pytest

from test_kernel_resources import HIPCC, _resources


@pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("c++filt") is None, reason="needs hipcc and c++filt")
def test_the_std_instances_keep_the_occupancy_of_the_instances_they_stand_beside():
    table = _resources("gsx_backward.hip")
    geometry, colour = table["backward_tile_geometry_kernel"], table["backward_tile_kernel"]
    std_geo, std_colour = table["backward_tile_std_geometry_kernel"], table["backward_tile_std_kernel"]
    print("std geometry", std_geo, "| geometry", geometry)
    print("std colour-only", std_colour, "| colour-only", colour)
    assert std_geo["ScratchSize"] == 0 and std_colour["ScratchSize"] == 0, (std_geo, std_colour)
    assert geometry["Occupancy"] >= 4, geometry                                   # what the merged tests hold it to
    assert std_geo["Occupancy"] >= geometry["Occupancy"], (std_geo, geometry)
    assert std_geo["LDS"] == geometry["LDS"] and std_colour["LDS"] == colour["LDS"], (std_geo, std_colour)
    assert std_colour["Occupancy"] >= colour["Occupancy"], (std_colour, colour)
    for kernel in ("backward_std_sum_kernel", "backward_std_chain_kernel", "backward_geometry_chain_kernel"):
        assert table[kernel]["ScratchSize"] == 0 and table[kernel]["LDS"] == 0, (kernel, table[kernel])
    assert table["backward_std_sum_kernel"]["VGPRs"] <= 32, table["backward_std_sum_kernel"]
    # the chain's std variant: one normalisation less, a radius more -- no more registers than the ref_cpu chain plus the radius
    assert table["backward_std_chain_kernel"]["VGPRs"] <= table["backward_geometry_chain_kernel"]["VGPRs"] + 8, table
    # the instances the older entries run, as the merged tests hold them
    depth, abs_ = table["backward_tile_depth_kernel"], table["backward_tile_abs_kernel"]
    assert colour["VGPRs"] <= 128 and colour["ScratchSize"] == 0 and colour["LDS"] == 4352, colour
    assert geometry["VGPRs"] <= 108 and geometry["ScratchSize"] == 0 and geometry["LDS"] == 5632, geometry
    assert depth["VGPRs"] <= 180 and depth["ScratchSize"] == 0 and depth["Occupancy"] >= 2 and depth["LDS"] == 6144, depth
    assert abs_["VGPRs"] <= 116 and abs_["ScratchSize"] == 0 and abs_["Occupancy"] >= 4, abs_
