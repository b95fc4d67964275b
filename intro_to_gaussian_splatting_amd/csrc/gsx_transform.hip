// gsx_transform_gaussians: a similarity transform x' = s R x + t of a Gaussian container, in place, in one launch.
//
// BUILD EXTENSION -- the reference has no such operation (its frame is whatever COLMAP wrote).  The formula and its float32
// operation order are the contract of include/gsx.h (gsx_transform_gaussians) and are restated op for op in
// tests/transform_restatement.py; the library is built with -ffp-contract=off, so every product and sum rounds on its own
// and the arrays are reproducible bit for bit from numpy:
//   points       p'_k = s ((R[k][0] x + R[k][1] y) + R[k][2] z) + t[k]
//   scales       c'_k = s c_k
//   quaternions  q' = q_R (x) q (Hamilton, (w, x, y, z)), each component three sums left to right, not renormalised
//   sh           band l = 1 .. DEG, every channel: sh'[l^2 + i] = sum_j M_l[i][j] sh[l^2 + j], the 2 l + 1 products summed
//                left to right; band 0 untouched
// The kernel derives nothing: R, s, t, q_R, M1, M2, M3 arrive as float32 in the kernel's argument (TransformArgs.T) and are
// read with scalar loads -- every index into them is a compile-time constant after unrolling.
//
// A pure stream: 2 x 4 x (10 + 3 K) bytes per row, K = (DEG + 1)^2 (464 B at degree 3, of which 384 are coefficients).  A
// workgroup owns kTransformRows = 256 consecutive rows (the block of adam_kernel, sh_backward_kernel and block_bounds).  Its
// coefficient run, 256 x 3 K contiguous floats, comes in through LDS exactly as sh_backward_kernel's does (sh::stage: 16-byte
// loads coalesced across the wave when the base is 16-byte aligned, single floats otherwise; padded rows of 3 K + 1 words,
// conflict free), every thread rotates the bands of its own row in LDS, and the run goes out through the same buffer
// (sh::unstage).  The block's run is complete in LDS (stage ends with a barrier) before anything of it is stored, and no other
// workgroup touches it: in place is safe.  The 10 floats of points, scales and quaternions are read and written by the row's
// own thread: a wave covers whole cache lines of each array.  The same operations on the same values on either path: the
// alignment of a base never changes a bit.  No atomics, no scratch.  Degree 3: 75 VGPRs, 49 KiB of LDS, three workgroups per
// CU; 0.092 ms for 10^6 rows on an MI355X = 5.06 TB/s, beside gsx_adam_step's 4.61 in the same session
// (tools/bench_transform.py; the table is in DESIGN.md section 8b, "Scene transforms").
#include "gsx_internal.h"
#include "gsx_sh_device.h"

namespace gsx {
namespace {

// Band L of one row (row: the thread's LDS row, 3 K + 1 words; M: (2 L + 1)^2 floats, row-major, in the kernel's argument).
template <int L>
__device__ __forceinline__ void rotate_band(float *row, const float *M) {
    constexpr int m = 2 * L + 1, o = L * L;
    float v[m][3];
#pragma unroll
    for (int j = 0; j < m; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) v[j][c] = row[3 * (o + j) + c];
#pragma unroll
    for (int i = 0; i < m; ++i)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float acc = M[i * m] * v[0][c];
#pragma unroll
            for (int j = 1; j < m; ++j) acc = acc + M[i * m + j] * v[j][c];
            row[3 * (o + i) + c] = acc;
        }
}

template <int DEG>
__global__ void __launch_bounds__(kTransformRows) transform_kernel(const TransformArgs k) {
    static_assert(kTransformRows == sh::kBlock, "sh::stage and sh::unstage move the block of sh::kBlock rows");
    __shared__ float lds[DEG > 0 ? sh::Layout<DEG>::kLdsFloats : 1];
    const int64_t g0 = (int64_t)blockIdx.x * kTransformRows;
    if (DEG > 0) sh::stage<DEG>(k.sh, k.n, g0, lds, k.vec != 0);
    const int64_t i = g0 + threadIdx.x;
    if (i < k.n) {
        const GsxTransform &T = k.T;
        float *p = k.points + 3 * i, *c = k.scales + 3 * i, *q = k.quats + 4 * i;
        const float x = p[0], y = p[1], z = p[2];
        const float c0 = c[0], c1 = c[1], c2 = c[2];
        const float bw = q[0], bx = q[1], by = q[2], bz = q[3];
        p[0] = T.s * ((T.R[0] * x + T.R[1] * y) + T.R[2] * z) + T.t[0];
        p[1] = T.s * ((T.R[3] * x + T.R[4] * y) + T.R[5] * z) + T.t[1];
        p[2] = T.s * ((T.R[6] * x + T.R[7] * y) + T.R[8] * z) + T.t[2];
        c[0] = T.s * c0;
        c[1] = T.s * c1;
        c[2] = T.s * c2;
        const float aw = T.q_R[0], ax = T.q_R[1], ay = T.q_R[2], az = T.q_R[3];
        q[0] = ((aw * bw - ax * bx) - ay * by) - az * bz;
        q[1] = ((aw * bx + ax * bw) + ay * bz) - az * by;
        q[2] = ((aw * by - ax * bz) + ay * bw) + az * bx;
        q[3] = ((aw * bz + ax * by) - ay * bx) + az * bw;
        if (DEG > 0) {
            float *row = lds + threadIdx.x * sh::Layout<DEG>::STRIDE;
            rotate_band<1>(row, T.M1);
            if (DEG > 1) rotate_band<2>(row, T.M2);
            if (DEG > 2) rotate_band<3>(row, T.M3);
        }
    }
    if (DEG > 0) sh::unstage<DEG>(k.sh, k.n, g0, lds, k.vec != 0);
}

}  // namespace

hipError_t launch_transform(const TransformArgs &args, int degree, hipStream_t s) {
    if (args.n <= 0) return hipSuccess;
    const int64_t nb = (args.n + kTransformRows - 1) / kTransformRows;
    if (nb > 0x7fffffff) return hipErrorInvalidValue;
    switch (degree) {
        case 0: transform_kernel<0><<<(unsigned)nb, kTransformRows, 0, s>>>(args); break;
        case 1: transform_kernel<1><<<(unsigned)nb, kTransformRows, 0, s>>>(args); break;
        case 2: transform_kernel<2><<<(unsigned)nb, kTransformRows, 0, s>>>(args); break;
        case 3: transform_kernel<3><<<(unsigned)nb, kTransformRows, 0, s>>>(args); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace gsx
