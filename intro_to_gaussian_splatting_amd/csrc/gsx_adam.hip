// gsx_adam_step: one Adam step over every parameter group of a Gaussian container, in one launch.
//
// BUILD EXTENSION -- the reference renders and stops; this is the update rule of the published 3D Gaussian Splatting
// trainer (Kerbl et al. 2023: Adam, scales stepped in log space, and the sparse variant that leaves Gaussians without a
// gradient alone).  The formula and its float32 operation order are the contract of include/gsx.h (gsx_adam_step) and are
// restated op for op in tests/adam_restatement.py; the library is built with -ffp-contract=off and correctly rounded divide
// and sqrt, so a LINEAR group's three arrays are reproducible bit for bit from numpy.
//
// A pure stream: 28 B per element of a row that is updated (gradient read; parameter and both moments read and written),
// 4 B per element of a row that GSX_ADAM_SKIP_ZERO_ROWS leaves alone.  A workgroup owns kAdamRows = 256 consecutive rows
// (the block sh_backward_kernel and block_bounds use): inside a group that is one contiguous run of 256 width floats, walked
// with 16-byte accesses when the group's four base pointers are 16-byte aligned (row0 width 4 B is a multiple of 1 KiB, so
// the run is aligned when the base is) and float by float otherwise.  The group descriptors are kernel arguments; the
// group index is uniform, so they are read with scalar loads.
//
// With the skip flag the workgroup first walks the gradient runs of all groups and marks, in a 256-entry LDS array, the
// rows that hold a non-zero bit pattern besides the sign (NaN is non-zero, -0 is zero); a marked row is stored as the same
// word by every lane that finds one, so no atomic is needed.  After the barrier the update walks the runs again -- the
// gradients of a block, at most a few hundred KiB, come from the cache the second time -- and touches only marked rows: a
// 16-byte group whose elements all lie in unmarked rows issues no load at all, one that straddles a marked and an unmarked
// row is done element by element.
#include "gsx_internal.h"

namespace gsx {
namespace {

__device__ __forceinline__ void adam_element(float &p, float g, float &m, float &v, bool log_space, float a,
                                             const AdamArgs &k) {
    const float gp = log_space ? g * p : g;             // dL/dtheta, theta = log p
    m = k.beta1 * m + k.c1 * gp;
    v = k.beta2 * v + (k.c2 * gp) * gp;
    const float d = sqrtf(v) / k.s2 + k.eps;
    const float u = a * (m / d);
    p = log_space ? p * expf(-u) : p - u;
}

__device__ __forceinline__ bool nonzero(float g) { return (__float_as_uint(g) & 0x7fffffffu) != 0u; }

template <bool SKIP>
__global__ void __launch_bounds__(kAdamRows) adam_kernel(const AdamArgs k) {
    __shared__ uint32_t live[SKIP ? kAdamRows : 1];
    const uint32_t tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * kAdamRows;
    const int64_t left = k.n - row0;
    const uint32_t rows = left < (int64_t)kAdamRows ? (uint32_t)left : (uint32_t)kAdamRows;

    if (SKIP) {
        live[tid] = 0u;
        __syncthreads();
        for (int gi = 0; gi < k.n_groups; ++gi) {
            const AdamGroupArgs &G = k.group[gi];
            const uint32_t w = (uint32_t)G.width, count = rows * w, nvec = G.vec ? count / 4u : 0u;
            const float *grad = G.grad + row0 * (int64_t)w;
            for (uint32_t q = tid; q < nvec; q += kAdamRows) {
                const float4 x = reinterpret_cast<const float4 *>(grad)[q];
                const float xs[4] = {x.x, x.y, x.z, x.w};
                uint32_t r = (4u * q) / w, rem = 4u * q - r * w;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (nonzero(xs[j])) live[r] = 1u;
                    if (++rem == w) { rem = 0u; ++r; }
                }
            }
            for (uint32_t e = 4u * nvec + tid; e < count; e += kAdamRows)
                if (nonzero(grad[e])) live[e / w] = 1u;
        }
        __syncthreads();
    }

    for (int gi = 0; gi < k.n_groups; ++gi) {
        const AdamGroupArgs &G = k.group[gi];
        const uint32_t w = (uint32_t)G.width, count = rows * w, nvec = G.vec ? count / 4u : 0u;
        const int64_t base = row0 * (int64_t)w;
        const float *grad = G.grad + base;
        float *param = G.param + base, *avg = G.exp_avg + base, *sq = G.exp_avg_sq + base;
        const bool log_space = G.log_space != 0;
        const float a = G.a;
        for (uint32_t q = tid; q < nvec; q += kAdamRows) {
            bool on[4] = {true, true, true, true};
            if (SKIP) {
                uint32_t r = (4u * q) / w, rem = 4u * q - r * w;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    on[j] = live[r] != 0u;
                    if (++rem == w) { rem = 0u; ++r; }
                }
            }
            if (on[0] && on[1] && on[2] && on[3]) {
                const float4 g4 = reinterpret_cast<const float4 *>(grad)[q];
                float4 p4 = reinterpret_cast<float4 *>(param)[q], m4 = reinterpret_cast<float4 *>(avg)[q],
                       v4 = reinterpret_cast<float4 *>(sq)[q];
                adam_element(p4.x, g4.x, m4.x, v4.x, log_space, a, k);
                adam_element(p4.y, g4.y, m4.y, v4.y, log_space, a, k);
                adam_element(p4.z, g4.z, m4.z, v4.z, log_space, a, k);
                adam_element(p4.w, g4.w, m4.w, v4.w, log_space, a, k);
                reinterpret_cast<float4 *>(param)[q] = p4;
                reinterpret_cast<float4 *>(avg)[q] = m4;
                reinterpret_cast<float4 *>(sq)[q] = v4;
            } else if (SKIP && (on[0] || on[1] || on[2] || on[3])) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (!on[j]) continue;
                    const uint32_t e = 4u * q + j;
                    float p = param[e], m = avg[e], v = sq[e];
                    adam_element(p, grad[e], m, v, log_space, a, k);
                    param[e] = p;
                    avg[e] = m;
                    sq[e] = v;
                }
            }
        }
        for (uint32_t e = 4u * nvec + tid; e < count; e += kAdamRows) {
            if (SKIP && live[e / w] == 0u) continue;
            float p = param[e], m = avg[e], v = sq[e];
            adam_element(p, grad[e], m, v, log_space, a, k);
            param[e] = p;
            avg[e] = m;
            sq[e] = v;
        }
    }
}

}  // namespace

hipError_t launch_adam(const AdamArgs &args, bool skip_zero_rows, hipStream_t s) {
    if (args.n <= 0) return hipSuccess;
    const int64_t nb = (args.n + kAdamRows - 1) / kAdamRows;
    if (nb > 0x7fffffff) return hipErrorInvalidValue;
    if (skip_zero_rows)
        adam_kernel<true><<<(unsigned)nb, kAdamRows, 0, s>>>(args);
    else
        adam_kernel<false><<<(unsigned)nb, kAdamRows, 0, s>>>(args);
    return hipGetLastError();
}

}  // namespace gsx
