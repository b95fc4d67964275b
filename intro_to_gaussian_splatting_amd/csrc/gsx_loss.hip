// The photometric loss of a splat fit, value and dL/dframe in one call (gsx_photometric_loss, include/gsx.h):
//   loss = (1 - lambda) mean|x - y| + lambda (1 - mean SSIM(x, y)),  11 x 11 Gaussian window, sigma 1.5, zero padding 5,
// over the rows x cols region at the origin of two channel-interleaved (.., .., 3) images, as if both were cropped to it.
//
// BUILD EXTENSION -- the reference renders and stops; the objective is the published one of 3D Gaussian Splatting
// (Kerbl et al. 2023) with the SSIM of Wang et al. 2004.  Parity is pinned to the float64 restatement of the formula
// (tests/photometric_loss_restatement.py) within 12 x the error torch's own float32 evaluation has against it.
//
// Three kernels, no atomics, every sum in a fixed order (same inputs, same bits):
//   loss_maps_kernel    gsx_loss_maps.inc, the instance without weight and exposure: m, |x - y| and -- with a gradient --
//                       w Dmu, w Dp, w Dq, w = -lambda / n; one (sum m, sum |x - y|) pair per workgroup
//   loss_reduce_kernel  one workgroup: the pairs summed in double (sum_records), loss_out = (loss, l1, ssim)
//   loss_grad_kernel    the same tiling: the three maps filtered (gsx_loss_grad_filter.inc), then combined with x, y and
//                       the L1 sign in a pass over whole interleaved rows
// Compiled with -ffp-contract=off; the filter taps are explicit fmaf chains.
// The two .inc texts and gsx_loss_device.h (tiling constants, Taps, stage_tile, block_sum, sum_records, LossLaunch) are
// shared with gsx_loss_weighted.hip.
#include "gsx_loss_device.h"

namespace gsx {
namespace {

template <bool GRAD>
__global__ void __launch_bounds__(NT)
    loss_maps_kernel(const float *__restrict__ image, int64_t image_stride, const float *__restrict__ target,
                     int64_t target_stride, int32_t R, int32_t C, Taps taps, float w, float *__restrict__ map_mu,
                     float *__restrict__ map_p, float *__restrict__ map_q, int64_t map_stride, float2 *__restrict__ partials,
                     uint32_t tiles_c, bool vec_x, bool vec_y) {
#define GSX_LOSS_WEIGHTED 0
#include "gsx_loss_maps.inc"
#undef GSX_LOSS_WEIGHTED
}

__global__ void __launch_bounds__(256)
    loss_reduce_kernel(const float2 *__restrict__ partials, int64_t tiles, double n, float lambda, float *__restrict__ loss_out) {
    __shared__ double sa[2][256];
    sum_records<2>(reinterpret_cast<const float *>(partials), tiles, sa);
    if (threadIdx.x == 0) {
        const double ssim = sa[0][0] / n, l1 = sa[1][0] / n, lam = (double)lambda;
        loss_out[0] = (float)((1.0 - lam) * l1 + lam * (1.0 - ssim));
        loss_out[1] = (float)l1;
        loss_out[2] = (float)ssim;
    }
}

__global__ void __launch_bounds__(NT)
    loss_grad_kernel(const float *__restrict__ image, int64_t image_stride, const float *__restrict__ target,
                     int64_t target_stride, float *__restrict__ grad, int64_t grad_stride, int32_t R, int32_t C, Taps taps,
                     float l1_weight, const float *__restrict__ map_mu, const float *__restrict__ map_p,
                     const float *__restrict__ map_q, int64_t map_stride, uint32_t tiles_c, bool vec_x, bool vec_y,
                     bool vec_g) {
#include "gsx_loss_grad_filter.inc"
    // F leaves through obuf[map][r][3 c + ch] over the staging area and meets x, y and the L1 sign a quad of a row at a time
    float *obuf = lds;
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
#pragma unroll
            for (int m = 0; m < PX; ++m) obuf[(k * T + tr + (NT / T) * m) * kRowFloats + 3 * tc + ch] = F[k][ch][m];
    __syncthreads();
    const int64_t lim = 3 * (int64_t)C;
    for (int idx = threadIdx.x; idx < T * kRowQuads; idx += NT) {
        const int r = idx / kRowQuads, q = idx % kRowQuads;
        const int64_t row = r0 + r, f0 = cf0 + 4 * q;
        if (row >= R || f0 >= lim) continue;
        const bool whole = f0 + 4 <= lim;
        const int cnt = whole ? 4 : (int)(lim - f0);
        const float *xs = image + row * image_stride + f0, *ys = target + row * target_stride + f0;
        float *gs = grad + row * grad_stride + f0;
        float x[4] = {0.0f, 0.0f, 0.0f, 0.0f}, y[4] = {0.0f, 0.0f, 0.0f, 0.0f}, g[4];
        if (whole && vec_x) {
            const float4 t = *reinterpret_cast<const float4 *>(xs);
            x[0] = t.x; x[1] = t.y; x[2] = t.z; x[3] = t.w;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e < cnt) x[e] = xs[e];
        }
        if (whole && vec_y) {
            const float4 t = *reinterpret_cast<const float4 *>(ys);
            y[0] = t.x; y[1] = t.y; y[2] = t.z; y[3] = t.w;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e < cnt) y[e] = ys[e];
        }
        const float4 fmu = *reinterpret_cast<const float4 *>(obuf + (0 * T + r) * kRowFloats + 4 * q);
        const float4 fp = *reinterpret_cast<const float4 *>(obuf + (1 * T + r) * kRowFloats + 4 * q);
        const float4 fq = *reinterpret_cast<const float4 *>(obuf + (2 * T + r) * kRowFloats + 4 * q);
        const float vmu[4] = {fmu.x, fmu.y, fmu.z, fmu.w}, vp[4] = {fp.x, fp.y, fp.z, fp.w}, vq[4] = {fq.x, fq.y, fq.z, fq.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float d = x[e] - y[e];
            const float sgn = (float)(d > 0.0f) - (float)(d < 0.0f);      // sign(0) = 0, as torch's abs
            g[e] = l1_weight * sgn + vmu[e] + (2.0f * x[e]) * vp[e] + y[e] * vq[e];
        }
        if (whole && vec_g) {
            *reinterpret_cast<float4 *>(gs) = make_float4(g[0], g[1], g[2], g[3]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e < cnt) gs[e] = g[e];
        }
    }
}

}  // namespace

hipError_t launch_photometric_loss(const LossImages &im, float lambda, float *loss_out, char *ws, const plan::LossCarve &c,
                                   hipStream_t s) {
    const Taps taps = window_taps();
    const double n = 3.0 * (double)im.rows * (double)im.cols;
    const float w = (float)(-(double)lambda / n), l1_weight = (float)((1.0 - (double)lambda) / n);
    const LossLaunch l = loss_launch(im, ws, c);
    float2 *partials = reinterpret_cast<float2 *>(ws + c.partials);
    hipError_t e = hipSuccess;
    if (l.run & 1) {
        if (im.grad)
            loss_maps_kernel<true><<<l.tiles, NT, 0, s>>>(im.image, im.image_stride, im.target, im.target_stride, im.rows, im.cols,
                                                          taps, w, l.mu, l.mp, l.mq, l.map_stride, partials, l.tiles_c, l.vx, l.vy);
        else
            loss_maps_kernel<false><<<l.tiles, NT, 0, s>>>(im.image, im.image_stride, im.target, im.target_stride, im.rows, im.cols,
                                                           taps, w, l.mu, l.mp, l.mq, l.map_stride, partials, l.tiles_c, l.vx, l.vy);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (l.run & 2) {
        loss_reduce_kernel<<<1, 256, 0, s>>>(partials, c.tiles, n, lambda, loss_out);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (im.grad && (l.run & 4)) {
        loss_grad_kernel<<<l.tiles, NT, 0, s>>>(im.image, im.image_stride, im.target, im.target_stride, im.grad, im.grad_stride,
                                                im.rows, im.cols, taps, l1_weight, l.mu, l.mp, l.mq, l.map_stride, l.tiles_c, l.vx,
                                                l.vy, l.vg);
        e = hipGetLastError();
    }
    return e;
}

}  // namespace gsx
