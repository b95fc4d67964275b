// gsx_density_accumulate_screen / gsx_density_plan_screen: density control on the published statistic -- the norm of
// dL/d(NDC mean) that gsx_render_backward_screen exports, counted over the frames that LISTED the Gaussian -- and the
// published second screen-space rule, pruning on the largest screen radius seen.
//
// The contract (rules, float32 operation order) is include/gsx.h's and is restated op for op in
// tests/screen_gradient_restatement.py; like gsx_density.hip this is built with -ffp-contract=off and correctly rounded
// divide and sqrt.  The plan is gsx_density_plan's: this file has the classify step with the radius comparison added, the
// scan of the block sums and the rows' places are gsx_density.hip's kernels (launch_density_plan_finish), so the
// workspace it leaves feeds the unchanged gsx_density_apply.
#include "gsx_density_device.h"

namespace gsx {
namespace {

using namespace density;

// One thread per row: 12 bytes read; a listed row (radius > 0; a NaN is not) reads and writes 12 more.
__global__ void __launch_bounds__(kThreads)
    density_accumulate_screen_kernel(const float *__restrict__ grad_means2d, const float *__restrict__ screen_radius, int64_t n,
                                     float *__restrict__ grad_sum, uint32_t *__restrict__ seen, float *__restrict__ radius_max) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const float r = screen_radius[i];
    if (!(r > 0.0f)) return;
    const float g0 = grad_means2d[2 * i], g1 = grad_means2d[2 * i + 1];     // (any float-aligned base: no 8-byte load)
    grad_sum[i] = grad_sum[i] + sqrtf(g0 * g0 + g1 * g1);
    seen[i] = seen[i] + 1u;
    const float old = radius_max[i];
    radius_max[i] = r > old ? r : old;
}

// density_classify_kernel with the radius rule: PRUNE also where radius_max[i] > prune_radius (a NaN fails it; radius_max
// null: the rule is off and the plan is gsx_density_plan's byte for byte).
__global__ void __launch_bounds__(kThreads)
    density_classify_screen_kernel(const float *__restrict__ grad_sum, const uint32_t *__restrict__ seen,
                                   const float *__restrict__ scales, const float *__restrict__ opacity_logit,
                                   const float *__restrict__ radius_max, float prune_radius, int64_t n, const GsxDensityRules rules,
                                   uint32_t *__restrict__ action4, uint32_t *__restrict__ bsum, uint32_t *__restrict__ bpruned,
                                   uint32_t *__restrict__ bsplit) {
    __shared__ uint32_t lds[kThreads];
    const int64_t r0 = (int64_t)blockIdx.x * kDensityScanRows + threadIdx.x * kScanPer;
    uint32_t word = 0u, out = 0u, tally = 0u;
#pragma unroll
    for (int k = 0; k < kScanPer; ++k) {
        uint32_t a = kDensityPrune;
        if (r0 + k < n) {
            a = classify(grad_sum, seen, scales, opacity_logit, r0 + k, rules);
            if (radius_max && radius_max[r0 + k] > prune_radius) a = kDensityPrune;
            out += rows_of(a);
            tally += (a == kDensityPrune ? 1u : 0u) + (a == kDensitySplit ? 0x10000u : 0u);
        }
        word |= a << (8 * k);
    }
    leave_block(word, out, tally, lds, action4, bsum, bpruned, bsplit);
}

}  // namespace

hipError_t launch_density_accumulate_screen(const float *grad_means2d, const float *screen_radius, int64_t n, float *grad_sum,
                                            uint32_t *seen, float *radius_max, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    density_accumulate_screen_kernel<<<(unsigned)((n + kThreads - 1) / kThreads), kThreads, 0, s>>>(
        grad_means2d, screen_radius, n, grad_sum, seen, radius_max);
    return hipGetLastError();
}

hipError_t launch_density_plan_screen(const float *grad_sum, const uint32_t *seen, const float *scales, const float *opacity_logit,
                                      const float *radius_max, float prune_radius, int64_t n, const GsxDensityRules &rules,
                                      char *ws, const DensityCarve &c, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const uint32_t nb = c.scan_blocks;
    uint32_t *action4 = reinterpret_cast<uint32_t *>(ws + c.action);
    uint32_t *bsum = reinterpret_cast<uint32_t *>(ws + c.bsum), *bpruned = bsum + nb + 1, *bsplit = bpruned + nb;
    density_classify_screen_kernel<<<nb, kThreads, 0, s>>>(grad_sum, seen, scales, opacity_logit, radius_max, prune_radius, n,
                                                           rules, action4, bsum, bpruned, bsplit);
    return launch_density_plan_finish(n, rules.split_shrink, ws, c, s);
}

}  // namespace gsx
