"""Register and scratch budget of the backward compositing kernel's three instances and of the depth kernels, from the
compiler's own report (tests/test_kernel_resources.py's helpers; hipcc cross-compiles: no GPU).  The colour-only and
the geometry instance are the ones the older entries run: the depth instance beside them must not move their registers,
their occupancy or give them scratch.  The depth instance carries six more floats per pixel (running and final D and A,
dL/dD, dL/dA: 24 registers for its four pixels) and may not use scratch; its register and occupancy figures are those of
the tree its timings were taken with."""
import os
import shutil

import pytest

from test_kernel_resources import HIPCC, _resources

DEPTH_TILE_VGPRS = 180      # backward_tile_depth_kernel as measured, left to the compiler's own occupancy
DEPTH_TILE_WAVES = 2
DEPTH_FORWARD_VGPRS = 64    # depth_tile_kernel


@pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("c++filt") is None, reason="needs hipcc and c++filt")
def test_backward_tile_instances_keep_their_budget_beside_the_depth_instance():
    table = _resources("gsx_backward.hip")
    colour, geometry, depth = (table[k] for k in ("backward_tile_kernel", "backward_tile_geometry_kernel", "backward_tile_depth_kernel"))
    print("colour-only", colour, "geometry", geometry, "depth", depth, "depth forward", table["depth_tile_kernel"])
    assert colour["VGPRs"] <= 128 and colour["ScratchSize"] == 0, colour
    assert geometry["VGPRs"] <= 108 and geometry["ScratchSize"] == 0 and geometry["Occupancy"] >= 4, geometry
    assert depth["ScratchSize"] == 0 and depth["VGPRs"] <= DEPTH_TILE_VGPRS and depth["Occupancy"] >= DEPTH_TILE_WAVES, depth
    forward = table["depth_tile_kernel"]
    assert forward["ScratchSize"] == 0 and forward["VGPRs"] <= DEPTH_FORWARD_VGPRS and forward["Occupancy"] >= 8, forward
    for kernel in ("backward_depth_sum_kernel", "backward_depth_chain_kernel"):
        assert table[kernel]["ScratchSize"] == 0, (kernel, table[kernel])
    assert table["backward_depth_chain_kernel"]["VGPRs"] <= 128
    assert _resources("gsx_project.hip")["project_depth_kernel"]["ScratchSize"] == 0
