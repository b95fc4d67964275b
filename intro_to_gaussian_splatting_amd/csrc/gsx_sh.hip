// View-dependent colour: real spherical harmonics (degree 0..3) -> RGB, one thread per Gaussian.
//
// BUILD EXTENSION -- the reference has no spherical harmonics at all (its colour is the stored
// rgb/256, splat/gaussians.py:20-22), so parity
// of this kernel is UNPINNED by the reference.  It follows the published 3D Gaussian Splatting
// convention (Kerbl et al. 2023, `eval_sh` of graphdeco-inria/gaussian-splatting, not part of
// /root/reference): colour = max(0, 0.5 + sum_k Y_k(d) * sh[k]), d = normalize(mean - camera
// centre), with the constants of gsx_sh_device.h.  Degree 0 with sh0 = (rgb - 0.5) / 0.28209479
// reproduces the reference's RGB path, which is how it is tested against the pinned pipeline.
//
// This file is the standalone entry (gsx_sh_to_rgb: colours for the stage-1 API) and its backward
// (gsx_sh_backward: the last link of the gradient chain of an SH scene).  The whole-path render
// evaluates the same code inside the projection kernel (GsxParams.sh), so a frame has no colour launch
// and no colour array at all.
//
// HBM-bound elementwise ops: 12 B (mean) + 12 (deg+1)^2 B (coefficients) read, 12 B written by the forward.
#include "gsx_internal.h"
#include "gsx_sh_device.h"

namespace gsx {
namespace {

template <int DEG>
__global__ void __launch_bounds__(sh::kBlock)
    sh_to_rgb_kernel(const float *__restrict__ means3d, const float *__restrict__ coeffs, int64_t n, float cx, float cy,
                     float cz, float *__restrict__ colors, bool vec) {
    __shared__ float lds[sh::Layout<DEG>::kLdsFloats];
    const int64_t g0 = (int64_t)blockIdx.x * sh::kBlock;
    sh::stage<DEG>(coeffs, n, g0, lds, vec);
    const int64_t i = g0 + threadIdx.x;
    if (i >= n) return;
    float r, g, b;
    sh::eval<DEG>(lds + threadIdx.x * sh::Layout<DEG>::STRIDE, means3d[3 * i] - cx, means3d[3 * i + 1] - cy,
                  means3d[3 * i + 2] - cz, r, g, b);
    colors[3 * i] = r;
    colors[3 * i + 1] = g;
    colors[3 * i + 2] = b;
}

// gsx_sh_backward: dL/dcolour -> dL/dsh and, through the view direction, dL/dmean.  The forward kernel's memory path
// mirrored: the workgroup's coefficient block comes in through LDS (sh::stage), every thread recomputes its Gaussian's
// pre-clamp colour with the forward's own operations (the mask: channels the forward did not clamp), takes what the mean
// gradient needs from its row, overwrites the row with Y_k * masked dL/dcolour, and the block goes out through the same
// LDS buffer as coalesced 16-byte stores (sh::unstage).  One row per thread, no atomics.
// HBM: 24 B + 24 K B per Gaussian (mean, dL/dcolour, coefficients in; coefficient gradients out), + 12 B for dL/dmean.
template <int DEG>
__global__ void __launch_bounds__(sh::kBlock)
    sh_backward_kernel(const float *__restrict__ means3d, const float *__restrict__ coeffs, int64_t n, float cx, float cy,
                       float cz, const float *__restrict__ grad_colors, float *__restrict__ grad_sh,
                       float *__restrict__ grad_means3d, bool vec_in, bool vec_out) {
    constexpr int K = sh::Layout<DEG>::K;
    __shared__ float lds[sh::Layout<DEG>::kLdsFloats];
    const int64_t g0 = (int64_t)blockIdx.x * sh::kBlock;
    sh::stage<DEG>(coeffs, n, g0, lds, vec_in);
    const int64_t i = g0 + threadIdx.x;
    if (i < n) {
        float *row = lds + threadIdx.x * sh::Layout<DEG>::STRIDE;
        float basis[K], x, y, z, inv, pre[3];
        sh::basis_at<DEG>(means3d[3 * i] - cx, means3d[3 * i + 1] - cy, means3d[3 * i + 2] - cz, basis, x, y, z, inv);
        sh::pre_clamp<DEG>(basis, row, pre[0], pre[1], pre[2]);
        float gm[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) gm[c] = pre[c] > 0.0f ? grad_colors[3 * i + c] : 0.0f;
        if (grad_means3d) {
            float gx = 0.0f, gy = 0.0f, gz = 0.0f;
            if (DEG > 0) {
                float t[K];
#pragma unroll
                for (int k = 0; k < K; ++k) t[k] = gm[0] * row[3 * k] + gm[1] * row[3 * k + 1] + gm[2] * row[3 * k + 2];
                float dgx, dgy, dgz;
                sh::basis_gradient<DEG>(t, x, y, z, dgx, dgy, dgz);
                const float radial = x * dgx + y * dgy + z * dgz;      // the part along d moves nothing: d stays a unit vector
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
    }
    sh::unstage<DEG>(grad_sh, n, g0, lds, vec_out);
}

}  // namespace

hipError_t launch_sh_backward(const float *means3d, const float *sh, int degree, int64_t n, const float *center,
                              const float *grad_colors, float *grad_sh, float *grad_means3d, hipStream_t s) {
    if (degree < 0 || degree > 3) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    const unsigned nb = (unsigned)((n + gsx::sh::kBlock - 1) / gsx::sh::kBlock);
    const float cx = center[0], cy = center[1], cz = center[2];
    const bool vi = (reinterpret_cast<uintptr_t>(sh) & 15u) == 0, vo = (reinterpret_cast<uintptr_t>(grad_sh) & 15u) == 0;
#define GSX_SH_BACKWARD(D) \
    sh_backward_kernel<D><<<nb, gsx::sh::kBlock, 0, s>>>(means3d, sh, n, cx, cy, cz, grad_colors, grad_sh, grad_means3d, vi, vo)
    switch (degree) {
        case 0: GSX_SH_BACKWARD(0); break;
        case 1: GSX_SH_BACKWARD(1); break;
        case 2: GSX_SH_BACKWARD(2); break;
        default: GSX_SH_BACKWARD(3); break;
    }
#undef GSX_SH_BACKWARD
    return hipGetLastError();
}

hipError_t launch_sh_to_rgb(const float *means3d, const float *sh, int degree, int64_t n, const float *center,
                            float *colors, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const unsigned nb = (unsigned)((n + gsx::sh::kBlock - 1) / gsx::sh::kBlock);
    const float cx = center[0], cy = center[1], cz = center[2];
    const bool vec = (reinterpret_cast<uintptr_t>(sh) & 15u) == 0;
    switch (degree) {
        case 0: sh_to_rgb_kernel<0><<<nb, gsx::sh::kBlock, 0, s>>>(means3d, sh, n, cx, cy, cz, colors, vec); break;
        case 1: sh_to_rgb_kernel<1><<<nb, gsx::sh::kBlock, 0, s>>>(means3d, sh, n, cx, cy, cz, colors, vec); break;
        case 2: sh_to_rgb_kernel<2><<<nb, gsx::sh::kBlock, 0, s>>>(means3d, sh, n, cx, cy, cz, colors, vec); break;
        case 3: sh_to_rgb_kernel<3><<<nb, gsx::sh::kBlock, 0, s>>>(means3d, sh, n, cx, cy, cz, colors, vec); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace gsx
