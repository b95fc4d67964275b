"""The per-Gaussian kernels of gsx_backward.hip -- the colour sums, the geometry sums and the chain -- are one body per role
behind a thin __global__ wrapper per variant.  The wrappers keep the names profiles, resource tables and the other
*_kernel_resources tests refer to, and what the compiler makes of the shared bodies is what it made of the copies they
replaced: scratch, LDS and waves per SIMD below are literals from the commit before the bodies were shared (its
tools/kres.py table, docs/lab_notes/per_gaussian_bodies.md).  VGPRs may move inside an allocation granule; these may not.

From the compiler's own report (tests/test_kernel_resources.py's helpers; hipcc cross-compiles: no GPU)."""
import os
import shutil

import pytest

from test_kernel_resources import HIPCC, _resources

needs_tools = pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("c++filt") is None, reason="needs hipcc and c++filt")

# kernel -> (scratch bytes per lane, LDS bytes per block, waves per SIMD)
PARENT = {
    "backward_sum_kernel": (0, 0, 8),
    "backward_std_sum_kernel": (0, 0, 8),
    "backward_std_aa_sum_kernel": (0, 0, 8),
    "backward_geometry_sum_kernel": (0, 0, 8),
    "backward_depth_sum_kernel": (0, 0, 8),
    "backward_geometry_abs_sum_kernel": (0, 0, 8),
    "backward_geometry_chain_kernel": (0, 0, 4),
    "backward_depth_chain_kernel": (0, 0, 4),
    "backward_std_chain_kernel": (0, 0, 4),
    "backward_std_aa_chain_kernel": (0, 0, 4),
    "backward_camera_chain_kernel": (0, 384, 4),     # 4 waves x 24 camera terms
}


@needs_tools
def test_the_compiled_object_holds_the_eleven_names():
    table = _resources("gsx_backward.hip")
    missing = sorted(set(PARENT) - set(table))
    assert not missing, (missing, sorted(table))
    assert len(table) == 22, sorted(table)      # the file's kernels: none added, none turned into a mangled template instance


@needs_tools
@pytest.mark.parametrize("kernel", sorted(PARENT))
def test_scratch_lds_and_occupancy_are_the_parents(kernel):
    r = _resources("gsx_backward.hip")[kernel]
    print(kernel, r)
    assert (r["ScratchSize"], r["LDS"], r["Occupancy"]) == PARENT[kernel], (kernel, r)
