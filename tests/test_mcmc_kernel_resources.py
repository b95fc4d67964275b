"""Scratch, LDS and register budget of the six kernels of csrc/gsx_mcmc.hip, from the compiler's own report (hipcc
cross-compiles: no GPU).  No scratch anywhere -- the apply kernel indexes its group descriptors inside the kernel-argument
segment with scalar loads, and its per-row table (source, moved, new opacity, scale factor: 5 KiB) and the 51 square roots
of the relocation live in LDS; the two per-step streams use no LDS at all; all six run at eight waves per SIMD.  These are
the figures of the build tools/bench_mcmc.py timed (the table in DESIGN.md section 8b, "Fixed-budget densification"): a
change that moves one is to be re-measured."""
import os
import shutil

import pytest

from test_kernel_resources import HIPCC, _resources

# kernel -> (max VGPRs, LDS bytes per workgroup as declared, min waves per SIMD); scratch is 0 for all
BUDGET = {
    "mcmc_regularize_kernel": (29, 0, 8),
    "mcmc_perturb_kernel<2>": (56, 0, 8),        # two rows per thread (four: 62 VGPRs, half the waves, 3.5 against 5.5 TB/s)
    "mcmc_weights_kernel": (26, 2048, 8),
    "mcmc_blocks_kernel": (30, 2048, 8),
    "mcmc_draw_kernel": (12, 0, 8),
    "mcmc_apply_kernel": (48, 5528, 8),          # source 1024 + moved 1024 + logit 1024 + factor 2048 + roots 408
}

needs_tools = pytest.mark.skipif(not os.path.exists(HIPCC) or shutil.which("c++filt") is None, reason="needs hipcc and c++filt")


@needs_tools
def test_mcmc_kernels_use_no_scratch():
    table = _resources("gsx_mcmc.hip")
    assert sorted(table) == sorted(BUDGET), sorted(table)
    for kernel, r in table.items():
        print(kernel, r)
        assert r["ScratchSize"] == 0, (kernel, r)


@needs_tools
@pytest.mark.parametrize("kernel", sorted(BUDGET))
def test_mcmc_kernels_stay_inside_their_measured_budget(kernel):
    vgprs, lds, occupancy = BUDGET[kernel]
    r = _resources("gsx_mcmc.hip")[kernel]
    assert r["VGPRs"] <= vgprs and r["LDS"] == lds and r["Occupancy"] >= occupancy, (kernel, r)
