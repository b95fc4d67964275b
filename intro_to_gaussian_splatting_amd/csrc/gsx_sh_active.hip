// The SH degree schedule: gsx_sh_to_rgb / gsx_sh_backward on the first (A+1)^2 coefficients of rows STORED at degree S > A
// (gsx_sh_to_rgb_active, gsx_sh_backward_active).  A fit trains the low bands first; its coefficient array, its gradient and
// its Adam moments keep the stored layout (n, (S+1)^2, 3) throughout, so nothing is packed, copied or scattered per step.
//
// The contract is the bits of the degree-A kernels of gsx_sh.hip on the packed array sh[:, :(A+1)^2]: the arithmetic is
// sh::basis_at<A>, sh::pre_clamp<A>, sh::eval<A> and sh::basis_gradient<A> of gsx_sh_device.h, in sh_backward_kernel's order,
// under the same -ffp-contract=off.  Only the memory path differs:
//   in   a strided gather, 12 K_A bytes every 12 K_S bytes, row by row into the padded LDS layout (sh::stage_rows' pattern);
//        the inactive coefficients are never read, so whatever they hold -- NaN included -- reaches no output;
//   out  (backward) the full degree-S row through sh::unstage<S>, the inactive tail written +0 in LDS first: every entry of
//        grad_sh is written, coalesced, as by gsx_sh_backward.
// The instances live here, not in gsx_sh.hip, whose kernels are pinned to their register and LDS figures.
// HBM per Gaussian: forward 24 + 12 K_A B; backward 24 + 12 K_A + 12 K_S B (+ 12 B for dL/dmean).
#include "gsx_internal.h"
#include "gsx_sh_device.h"

namespace gsx {
namespace {

// The workgroup's rows [g0, g0 + 256) of the degree-S array: the first 3 K_A floats of each into lds[r * STRIDE + c], consecutive
// lanes on consecutive floats of a row.  16-byte loads where every row's active part starts and ends on one: both row widths
// a multiple of 4 floats -- (A, S) = (1, 3) only -- and the base aligned (vec).  Ends with a barrier: every thread calls it.
template <int A, int S, int STRIDE>
__device__ __forceinline__ void stage_active(const float *__restrict__ coeffs, int64_t n, int64_t g0, float *lds, bool vec) {
    constexpr int WA = sh::Layout<A>::W, WS = sh::Layout<S>::W;
    const int64_t left = n - g0 > 0 ? n - g0 : 0;
    const int rows = (int)(left < sh::kBlock ? left : sh::kBlock);
    const float *src = coeffs + (size_t)g0 * WS;
    if (WA % 4 == 0 && WS % 4 == 0 && vec) {
        constexpr int Q = WA % 4 == 0 ? WA / 4 : 1;
        for (int v = threadIdx.x; v < rows * Q; v += sh::kBlock) {
            const int r = v / Q, q = v % Q;
            const float4 f = *reinterpret_cast<const float4 *>(src + (size_t)r * WS + 4 * q);
            float *d = lds + r * STRIDE + 4 * q;
            d[0] = f.x; d[1] = f.y; d[2] = f.z; d[3] = f.w;
        }
    } else {
        for (int v = threadIdx.x; v < rows * WA; v += sh::kBlock) {
            const int r = v / WA, c = v % WA;
            lds[r * STRIDE + c] = src[(size_t)r * WS + c];
        }
    }
    __syncthreads();
}

template <int A, int S>
__global__ void __launch_bounds__(sh::kBlock)
    sh_to_rgb_active_kernel(const float *__restrict__ means3d, const float *__restrict__ coeffs, int64_t n, float cx, float cy,
                            float cz, float *__restrict__ colors, bool vec) {
    static_assert(A < S, "A == S is gsx_sh.hip's kernel");
    constexpr int STRIDE = sh::Layout<A>::STRIDE;
    __shared__ float lds[sh::Layout<A>::kLdsFloats];
    const int64_t g0 = (int64_t)blockIdx.x * sh::kBlock;
    stage_active<A, S, STRIDE>(coeffs, n, g0, lds, vec);
    const int64_t i = g0 + threadIdx.x;
    if (i >= n) return;
    float r, g, b;
    sh::eval<A>(lds + threadIdx.x * STRIDE, means3d[3 * i] - cx, means3d[3 * i + 1] - cy, means3d[3 * i + 2] - cz, r, g, b);
    colors[3 * i] = r;
    colors[3 * i + 1] = g;
    colors[3 * i + 2] = b;
}

// sh_backward_kernel<A> (gsx_sh.hip), statement for statement, on rows of the degree-S pitch: the LDS buffer is the degree-S
// one, a thread's row holds its 3 K_A active coefficients in front, and what goes out is the whole row.
template <int A, int S>
__global__ void __launch_bounds__(sh::kBlock)
    sh_backward_active_kernel(const float *__restrict__ means3d, const float *__restrict__ coeffs, int64_t n, float cx, float cy,
                              float cz, const float *__restrict__ grad_colors, float *__restrict__ grad_sh,
                              float *__restrict__ grad_means3d, bool vec_in, bool vec_out) {
    static_assert(A < S, "A == S is gsx_sh.hip's kernel");
    constexpr int K = sh::Layout<A>::K, WA = sh::Layout<A>::W, WS = sh::Layout<S>::W, STRIDE = sh::Layout<S>::STRIDE;
    __shared__ float lds[sh::Layout<S>::kLdsFloats];
    const int64_t g0 = (int64_t)blockIdx.x * sh::kBlock;
    stage_active<A, S, STRIDE>(coeffs, n, g0, lds, vec_in);
    const int64_t i = g0 + threadIdx.x;
    if (i < n) {
        float *row = lds + threadIdx.x * STRIDE;
        float basis[K], x, y, z, inv, pre[3];
        sh::basis_at<A>(means3d[3 * i] - cx, means3d[3 * i + 1] - cy, means3d[3 * i + 2] - cz, basis, x, y, z, inv);
        sh::pre_clamp<A>(basis, row, pre[0], pre[1], pre[2]);
        float gm[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) gm[c] = pre[c] > 0.0f ? grad_colors[3 * i + c] : 0.0f;
        if (grad_means3d) {
            float gx = 0.0f, gy = 0.0f, gz = 0.0f;
            if (A > 0) {
                float t[K];
#pragma unroll
                for (int k = 0; k < K; ++k) t[k] = gm[0] * row[3 * k] + gm[1] * row[3 * k + 1] + gm[2] * row[3 * k + 2];
                float dgx, dgy, dgz;
                sh::basis_gradient<A>(t, x, y, z, dgx, dgy, dgz);
                const float radial = x * dgx + y * dgy + z * dgz;
                gx = (dgx - x * radial) * inv;
                gy = (dgy - y * radial) * inv;
                gz = (dgz - z * radial) * inv;
                // The zero-row rule (include/gsx.h): without a non-zero masked dL/dcolour nothing of the row's own reaches
                // dL/dmean.  A row the frame listed nowhere has gm = 0, and its mean may be NaN, infinite or the camera
                // centre itself, or a coefficient NaN: 0 * NaN above is NaN, and the caller sums every row's share into
                // the pose's gradient.  (A select on a wave mask: no register is held for it.)
                if (gm[0] == 0.0f && gm[1] == 0.0f && gm[2] == 0.0f) gx = gy = gz = 0.0f;
            }
            grad_means3d[3 * i] = gx;
            grad_means3d[3 * i + 1] = gy;
            grad_means3d[3 * i + 2] = gz;
        }
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) row[3 * k + c] = pre[c] > 0.0f ? basis[k] * gm[c] : 0.0f;
#pragma unroll
        for (int c = WA; c < WS; ++c) row[c] = 0.0f;        // the inactive bands: exact +0
    }
    sh::unstage<S>(grad_sh, n, g0, lds, vec_out);
}

bool degrees_ok(int stored, int active) { return stored >= 0 && stored <= 3 && active >= 0 && active <= stored; }

}  // namespace

hipError_t launch_sh_to_rgb_active(const float *means3d, const float *sh, int stored, int active, int64_t n,
                                   const float *center, float *colors, hipStream_t s) {
    if (!degrees_ok(stored, active)) return hipErrorInvalidValue;
    if (active == stored) return launch_sh_to_rgb(means3d, sh, stored, n, center, colors, s);
    if (n == 0) return hipSuccess;
    const unsigned nb = (unsigned)((n + gsx::sh::kBlock - 1) / gsx::sh::kBlock);
    const float cx = center[0], cy = center[1], cz = center[2];
    const bool vec = (reinterpret_cast<uintptr_t>(sh) & 15u) == 0;
#define GSX_SH_ACTIVE(A, S) \
    sh_to_rgb_active_kernel<A, S><<<nb, gsx::sh::kBlock, 0, s>>>(means3d, sh, n, cx, cy, cz, colors, vec)
    switch (4 * stored + active) {
        case 4 * 1 + 0: GSX_SH_ACTIVE(0, 1); break;
        case 4 * 2 + 0: GSX_SH_ACTIVE(0, 2); break;
        case 4 * 2 + 1: GSX_SH_ACTIVE(1, 2); break;
        case 4 * 3 + 0: GSX_SH_ACTIVE(0, 3); break;
        case 4 * 3 + 1: GSX_SH_ACTIVE(1, 3); break;
        default: GSX_SH_ACTIVE(2, 3); break;
    }
#undef GSX_SH_ACTIVE
    return hipGetLastError();
}

hipError_t launch_sh_backward_active(const float *means3d, const float *sh, int stored, int active, int64_t n,
                                     const float *center, const float *grad_colors, float *grad_sh, float *grad_means3d,
                                     hipStream_t s) {
    if (!degrees_ok(stored, active)) return hipErrorInvalidValue;
    if (active == stored) return launch_sh_backward(means3d, sh, stored, n, center, grad_colors, grad_sh, grad_means3d, s);
    if (n == 0) return hipSuccess;
    const unsigned nb = (unsigned)((n + gsx::sh::kBlock - 1) / gsx::sh::kBlock);
    const float cx = center[0], cy = center[1], cz = center[2];
    const bool vi = (reinterpret_cast<uintptr_t>(sh) & 15u) == 0, vo = (reinterpret_cast<uintptr_t>(grad_sh) & 15u) == 0;
#define GSX_SH_ACTIVE(A, S)                                                                                             \
    sh_backward_active_kernel<A, S><<<nb, gsx::sh::kBlock, 0, s>>>(means3d, sh, n, cx, cy, cz, grad_colors, grad_sh, \
                                                                   grad_means3d, vi, vo)
    switch (4 * stored + active) {
        case 4 * 1 + 0: GSX_SH_ACTIVE(0, 1); break;
        case 4 * 2 + 0: GSX_SH_ACTIVE(0, 2); break;
        case 4 * 2 + 1: GSX_SH_ACTIVE(1, 2); break;
        case 4 * 3 + 0: GSX_SH_ACTIVE(0, 3); break;
        case 4 * 3 + 1: GSX_SH_ACTIVE(1, 3); break;
        default: GSX_SH_ACTIVE(2, 3); break;
    }
#undef GSX_SH_ACTIVE
    return hipGetLastError();
}

}  // namespace gsx
