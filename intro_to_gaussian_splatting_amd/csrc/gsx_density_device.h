// Device code the plan kernels of gsx_density.hip and gsx_density_screen.hip share: a row's action under the rules of
// gsx_density_plan (include/gsx.h), its output rows, and the workgroup scan both classify kernels end with.
#pragma once

#include "gsx_internal.h"

namespace gsx {
namespace density {

constexpr int kThreads = 256, kScanPer = kDensityScanRows / kThreads;
static_assert(kScanPer == 4, "a thread packs its four action bytes into one word");

__device__ __forceinline__ uint32_t rows_of(uint32_t action) {
    return action == kDensityPrune ? 0u : (action == kDensityKeep ? 1u : 2u);
}

// max(a, b) that is NaN when either is
__device__ __forceinline__ float max_nan(float a, float b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }

// Exclusive scan of one value per thread over the 256 threads of the workgroup; total = the sum.
__device__ __forceinline__ uint32_t block_exclusive(uint32_t v, uint32_t *lds, uint32_t &total) {
    const int t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
#pragma unroll
    for (int s = 1; s < kThreads; s <<= 1) {
        const uint32_t add = t >= s ? lds[t - s] : 0u;
        __syncthreads();
        lds[t] += add;
        __syncthreads();
    }
    total = lds[kThreads - 1];
    const uint32_t incl = lds[t];
    __syncthreads();
    return incl - v;
}

__device__ __forceinline__ uint32_t classify(const float *__restrict__ grad_sum, const uint32_t *__restrict__ seen,
                                             const float *__restrict__ scales, const float *__restrict__ opacity_logit,
                                             int64_t i, const GsxDensityRules &r) {
    const float smax = max_nan(max_nan(scales[3 * i], scales[3 * i + 1]), scales[3 * i + 2]);
    if (opacity_logit[i] < r.prune_logit || smax > r.prune_scale) return kDensityPrune;
    const uint32_t c = seen[i];
    if (c > 0u && grad_sum[i] / (float)c >= r.grad_threshold) {
        if (smax > r.dense_scale) return kDensitySplit;
        if (smax <= r.dense_scale) return kDensityClone;
    }
    return kDensityKeep;
}

// What a classify kernel leaves of its 1024 rows: the thread's four action bytes, then the block's output rows, pruned and
// split rows.  out: the thread's output rows; tally: pruned | split << 16 (each at most 1024 in a block).
__device__ __forceinline__ void leave_block(uint32_t word, uint32_t out, uint32_t tally, uint32_t *lds,
                                            uint32_t *__restrict__ action4, uint32_t *__restrict__ bsum,
                                            uint32_t *__restrict__ bpruned, uint32_t *__restrict__ bsplit) {
    action4[(size_t)blockIdx.x * kThreads + threadIdx.x] = word;
    uint32_t total, total2;
    (void)block_exclusive(out, lds, total);
    (void)block_exclusive(tally, lds, total2);
    if (threadIdx.x == 0) {
        bsum[blockIdx.x] = total;
        bpruned[blockIdx.x] = total2 & 0xffffu;
        bsplit[blockIdx.x] = total2 >> 16;
    }
}

}  // namespace density
}  // namespace gsx
