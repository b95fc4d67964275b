"""Register, scratch and LDS budget around GSX_FLAG_ANTIALIASED, from the compiler's own report
(tests/test_kernel_resources.py's helpers; hipcc cross-compiles: no GPU).

The flag changes what stage 1 packs and what two per-Gaussian kernels do; nothing per (pixel, Gaussian) pair.  So the kernels
a flag-clear call runs keep the figures they had before the flag existed -- the two std_3dgs backward tile instances, the
std_3dgs compositing kernels, the projection instances, the std sum and chain kernels: recorded below from the commit that
added the flag, equal to its parent's -- and the anti-aliased instances stand beside them: no scratch, and no occupancy below
the instance they derive from."""
import os
import shutil

import pytest

from test_kernel_resources import HIPCC, _resources

needs_tools = pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("c++filt") is None, reason="needs hipcc and c++filt")

# kernel -> (VGPRs, scratch bytes per lane, LDS bytes per block): what the flag-clear call ran before and runs now
UNCHANGED = {
    "gsx_backward.hip": {
        "backward_tile_std_geometry_kernel": (120, 0, 5632),
        "backward_tile_std_kernel": (110, 0, 4352),
        "backward_std_sum_kernel": (16, 0, 0),
        "backward_std_chain_kernel": (114, 0, 0),
    },
    "gsx_blend.hip": {
        "blend_std16_kernel": (64, 20, 3632),         # (its 20 bytes of scratch are older than the flag)
        "blend_rules_kernel<2>": (32, 0, 4096),
    },
    "gsx_project.hip": {
        "project_pack_kernel<false, -1>": (46, 0, 9260),
        "project_window_kernel<false, -1>": (72, 0, 9788),
    },
    "gsx_contribution.hip": {
        "contribution_tile_std_kernel": (48, 0, 3072),
    },
}


@needs_tools
@pytest.mark.parametrize("src", sorted(UNCHANGED))
def test_the_kernels_of_a_flag_clear_call_keep_their_figures(src):
    table = _resources(src)
    for kernel, (vgprs, scratch, lds) in UNCHANGED[src].items():
        r = table[kernel]
        print(kernel, r)
        assert (r["VGPRs"], r["ScratchSize"], r["LDS"]) == (vgprs, scratch, lds), (kernel, r)


@needs_tools
def test_the_antialiased_instances_use_no_scratch_and_keep_the_occupancy():
    back, proj = _resources("gsx_backward.hip"), _resources("gsx_project.hip")
    chain, aa_chain = back["backward_std_chain_kernel"], back["backward_std_aa_chain_kernel"]
    sums, aa_sums = back["backward_std_sum_kernel"], back["backward_std_aa_sum_kernel"]
    print("chain", chain, "| antialiased", aa_chain)
    print("sum", sums, "| antialiased", aa_sums)
    assert aa_chain["ScratchSize"] == 0 and aa_chain["LDS"] == 0 and aa_chain["Occupancy"] >= chain["Occupancy"]
    assert aa_chain["VGPRs"] <= chain["VGPRs"] + 8          # two more covariance entries, U and three quotients
    assert aa_sums["ScratchSize"] == 0 and aa_sums["LDS"] == 0 and aa_sums["VGPRs"] <= 32
    assert aa_sums["Occupancy"] >= sums["Occupancy"]
    pairs = [(k, k.replace("_kernel<", "_aa_kernel<")) for k in proj if k.startswith(("project_pack_kernel<", "project_window_kernel<"))]
    assert len(pairs) == 20                                 # two kernels, device camera or not, RGB and four SH degrees
    for plain, aa in pairs:
        assert aa in proj, aa
        assert proj[aa]["ScratchSize"] == 0 and proj[aa]["LDS"] == proj[plain]["LDS"], (aa, proj[aa])
        # (rho and the two undilated entries stay live across the rectangle: at most one wave per SIMD fewer)
        assert proj[aa]["Occupancy"] >= proj[plain]["Occupancy"] - 1, (aa, proj[aa], proj[plain])
    # the frame's own instance: the occupancy the merged budget holds the flag-clear one to
    assert proj["project_pack_aa_kernel<false, -1>"]["Occupancy"] >= 7 and proj["project_window_aa_kernel<false, -1>"]["Occupancy"] >= 6
