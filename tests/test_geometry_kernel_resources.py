"""Register and scratch budget of the backward compositing kernel's two instances, from the compiler's own report
(tests/test_kernel_resources.py's helpers; hipcc cross-compiles: no GPU).  The colour-only instance is the one
gsx_render_backward has always run: adding the geometry instance beside it must not move its registers or give it
scratch.  The geometry instance (five more sums per record) must stay free of scratch."""
import os
import shutil

import pytest

from test_kernel_resources import HIPCC, _resources

COLOUR_ONLY_VGPRS = 128     # backward_tile_kernel before its walk became a template, and since


@pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("c++filt") is None, reason="needs hipcc and c++filt")
def test_backward_tile_instances_keep_their_budget():
    table = _resources("gsx_backward.hip")
    colour, geometry = table["backward_tile_kernel"], table["backward_tile_geometry_kernel"]
    print("colour-only", colour, "geometry", geometry)
    assert colour["VGPRs"] == COLOUR_ONLY_VGPRS and colour["ScratchSize"] == 0 and colour["Occupancy"] >= 4, colour
    assert geometry["ScratchSize"] == 0, geometry
    for kernel in ("backward_geometry_sum_kernel", "backward_geometry_chain_kernel"):
        assert table[kernel]["ScratchSize"] == 0, (kernel, table[kernel])
    assert table["backward_sum_kernel"]["ScratchSize"] == 0
