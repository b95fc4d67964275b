"""Register, scratch and LDS budget of gsx_sh_backward's four degree instances, from the compiler's own report
(tests/test_kernel_resources.py's helpers; hipcc cross-compiles: no GPU).  The kernel keeps a Gaussian's basis (K values)
and, for the mean gradient, K coefficient sums in registers: neither may spill.  Its LDS is the forward's one staging
buffer, used in both directions -- at most sh::Layout<3>::kLdsFloats floats -- so as many workgroups fit a CU as the
forward's.  The VGPR counts are what the build gave when the kernel was measured; one that grows is to be measured again."""
import os
import shutil

import pytest

from test_kernel_resources import HIPCC, _resources

K_BLOCK = 256
LDS_FLOATS_DEGREE_3 = K_BLOCK * (3 * 16 + 1)      # sh::Layout<3>::kLdsFloats: 256 rows at the padded stride of 49 words
VGPRS = {0: 18, 1: 34, 2: 64, 3: 102}


@pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("c++filt") is None, reason="needs hipcc and c++filt")
def test_sh_backward_instances_keep_their_budget():
    table = _resources("gsx_sh.hip")
    for degree, vgprs in VGPRS.items():
        r = table["sh_backward_kernel<%d>" % degree]
        print("degree", degree, r)
        assert r["ScratchSize"] == 0, (degree, r)
        assert r["LDS"] <= LDS_FLOATS_DEGREE_3 * 4, (degree, r)
        assert r["LDS"] == K_BLOCK * (3 * (degree + 1) ** 2 + 1) * 4, (degree, r)      # ONE buffer, in and out
        assert r["VGPRs"] <= vgprs, (degree, r)
    # the forward beside it keeps the LDS it had
    for degree in range(4):
        assert table["sh_to_rgb_kernel<%d>" % degree]["LDS"] == table["sh_backward_kernel<%d>" % degree]["LDS"]
