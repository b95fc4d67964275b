// The photometric loss with a per-pixel weight m and a per-view exposure E (gsx_photometric_loss_weighted, include/gsx.h):
//   x'_i = ((E_i0 x_0 + E_i1 x_1) + E_i2 x_2) + E_i3 inside the region, 0 outside;  W = sum m
//   loss = (1 - lambda) sum m |x' - y| / (3 W) + lambda (1 - sum m SSIM-map(x', y) / (3 W))
// value, dL/dimage and dL/dE in one call.  The tiling, the staging, the filter and the maps are gsx_loss.hip's, from the
// same texts (gsx_loss_device.h, gsx_loss_maps.inc, gsx_loss_grad_filter.inc); what is this file's own is where the weight
// and the exposure enter, and that 1 / W is not known while the maps are formed:
//   wloss_maps_kernel             gsx_loss_maps.inc, the instance with weight and exposure.  Stores m Dmu, m Dp, m Dq
//                                 UNSCALED and three sums per workgroup: sum m, sum m ssim-map, sum m |x' - y|
//   wloss_reduce_kernel           one workgroup: the sums in double (sum_records); loss_out = (loss, l1, ssim, W) and, for the
//                                 gradient kernel, (1 - lambda) / (3 W) and -lambda / (3 W) in the workspace (+0 when W == 0):
//                                 W never reaches the host
//   wloss_grad_kernel             the three maps filtered (gsx_loss_grad_filter.inc); each thread then forms g' of its own
//                                 pixels from the scales, m, x' and y, dL/dx = E[:, :3]^T g' (which leaves through LDS as whole
//                                 interleaved rows), and its share of the twelve sums of dL/dE: down the lanes of a wave,
//                                 then the waves in turn, twelve partials per workgroup
//   wloss_exposure_reduce_kernel  one workgroup: the partials in double, in sum_records' order
// No atomics; same inputs, same bits.  Compiled with -ffp-contract=off: x' is rounded product by product as written.
#include "gsx_loss_device.h"

namespace gsx {
namespace {

constexpr int kSums = plan::kLossWeightedSums, kTerms = plan::kLossExposureTerms;
static_assert(kSums == 3 && kTerms == 12 && plan::kLossScaleFloats >= 3, "the indices below");

struct Exposure {
    float e[kTerms];        // row-major 3 x 4
};

__device__ __forceinline__ Exposure load_exposure(const float *__restrict__ exposure) {
    Exposure E;
#pragma unroll
    for (int k = 0; k < kTerms; ++k) E.e[k] = exposure[k];
    return E;
}

// x' of one pixel, in the order of include/gsx.h.
__device__ __forceinline__ void expose(const Exposure &E, float x0, float x1, float x2, float out[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) out[i] = ((E.e[4 * i] * x0 + E.e[4 * i + 1] * x1) + E.e[4 * i + 2] * x2) + E.e[4 * i + 3];
}

template <bool GRAD, bool EXPO>
__global__ void __launch_bounds__(NT)
    wloss_maps_kernel(const float *__restrict__ image, int64_t image_stride, const float *__restrict__ target,
                      int64_t target_stride, const float *__restrict__ weight, int64_t weight_stride,
                      const float *__restrict__ exposure, int32_t R, int32_t C, Taps taps, float *__restrict__ map_mu,
                      float *__restrict__ map_p, float *__restrict__ map_q, int64_t map_stride, float *__restrict__ sums,
                      uint32_t tiles_c, bool vec_x, bool vec_y) {
#define GSX_LOSS_WEIGHTED 1
#include "gsx_loss_maps.inc"
#undef GSX_LOSS_WEIGHTED
}

__global__ void __launch_bounds__(256)
    wloss_reduce_kernel(const float *__restrict__ sums, int64_t tiles, float lambda, float *__restrict__ loss_out,
                        float *__restrict__ scale) {
    __shared__ double sa[kSums][256];
    sum_records<kSums>(sums, tiles, sa);
    if (threadIdx.x == 0) {
        const double W = sa[0][0], lam = (double)lambda;
        float out[4] = {0.0f, 0.0f, 0.0f, 0.0f}, l1_weight = 0.0f, w = 0.0f;
        if (W > 0.0) {          // (a NaN fails the comparison: weights are finite and >= 0 by contract)
            const double n = 3.0 * W, ssim = sa[1][0] / n, l1 = sa[2][0] / n;
            out[0] = (float)((1.0 - lam) * l1 + lam * (1.0 - ssim));
            out[1] = (float)l1;
            out[2] = (float)ssim;
            out[3] = (float)W;
            l1_weight = (float)((1.0 - lam) / n);
            w = (float)(-lam / n);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) loss_out[k] = out[k];
        scale[0] = l1_weight;
        scale[1] = w;
        scale[2] = out[3];
        scale[3] = 0.0f;
    }
}

template <bool EXPO>
__global__ void __launch_bounds__(NT)
    wloss_grad_kernel(const float *__restrict__ image, int64_t image_stride, const float *__restrict__ target,
                      int64_t target_stride, const float *__restrict__ weight, int64_t weight_stride,
                      const float *__restrict__ exposure, float *__restrict__ grad, int64_t grad_stride, int32_t R, int32_t C,
                      Taps taps, const float *__restrict__ scale, const float *__restrict__ map_mu,
                      const float *__restrict__ map_p, const float *__restrict__ map_q, int64_t map_stride,
                      float *__restrict__ exposure_partials, uint32_t tiles_c, bool vec_g) {
#include "gsx_loss_grad_filter.inc"
    // g' and dL/dx of this thread's own pixels; the rows leave through obuf[r][3 c + ch] over the staging area
    const float l1_weight = scale[0], w = scale[1];
    const bool dead = !(scale[2] > 0.0f);          // W == 0: every gradient is an exact +0
    Exposure E;
    if (EXPO) E = load_exposure(exposure);
    float acc[kTerms];
#pragma unroll
    for (int k = 0; k < kTerms; ++k) acc[k] = 0.0f;
    float *obuf = lds;
#pragma unroll
    for (int m = 0; m < PX; ++m) {
        const int r = tr + (NT / T) * m;
        const int64_t row = r0 + r, col = c0 + tc;
        float gx[3] = {0.0f, 0.0f, 0.0f};
        if (row < R && col < C && !dead) {
            const float *xs = image + row * image_stride + 3 * col, *ys = target + row * target_stride + 3 * col;
            const float x[3] = {xs[0], xs[1], xs[2]}, y[3] = {ys[0], ys[1], ys[2]};
            const float mv = weight ? weight[row * weight_stride + col] : 1.0f;
            float xp[3] = {x[0], x[1], x[2]}, gp[3];
            if (EXPO) expose(E, x[0], x[1], x[2], xp);
            const float l1m = l1_weight * mv;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const float d = xp[ch] - y[ch];
                const float sgn = (float)(d > 0.0f) - (float)(d < 0.0f);      // sign(0) = 0, as torch's abs
                gp[ch] = l1m * sgn + w * F[0][ch][m] + (2.0f * xp[ch]) * (w * F[1][ch][m]) + y[ch] * (w * F[2][ch][m]);
            }
            if (EXPO) {
#pragma unroll
                for (int j = 0; j < 3; ++j) gx[j] = (E.e[j] * gp[0] + E.e[4 + j] * gp[1]) + E.e[8 + j] * gp[2];
#pragma unroll
                for (int i = 0; i < 3; ++i) {
#pragma unroll
                    for (int j = 0; j < 3; ++j) acc[4 * i + j] += gp[i] * x[j];
                    acc[4 * i + 3] += gp[i];
                }
            } else {
#pragma unroll
                for (int j = 0; j < 3; ++j) gx[j] = gp[j];
            }
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) obuf[r * kRowFloats + 3 * tc + ch] = gx[ch];
    }
    if (EXPO && exposure_partials) {
        // twelve sums in a fixed order: down the lanes of a wave, then the waves in turn (hp does not overlap obuf)
#pragma unroll
        for (int k = 0; k < kTerms; ++k) {
            float v = acc[k];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
            if ((threadIdx.x & 63) == 0) hp[(threadIdx.x >> 6) * kTerms + k] = v;
        }
    }
    __syncthreads();
    if (EXPO && exposure_partials && threadIdx.x < kTerms) {
        float s = 0.0f;
        for (int k = 0; k < NT / 64; ++k) s += hp[k * kTerms + threadIdx.x];
        exposure_partials[(size_t)blockIdx.x * kTerms + threadIdx.x] = s;
    }
    const int64_t lim = 3 * (int64_t)C;
    for (int idx = threadIdx.x; idx < T * kRowQuads; idx += NT) {
        const int r = idx / kRowQuads, q = idx % kRowQuads;
        const int64_t row = r0 + r, f0 = cf0 + 4 * q;
        if (row >= R || f0 >= lim) continue;
        float *dst = grad + row * grad_stride + f0;
        const float *src = obuf + r * kRowFloats + 4 * q;
        if (f0 + 4 <= lim && vec_g) {
            *reinterpret_cast<float4 *>(dst) = *reinterpret_cast<const float4 *>(src);
        } else {
            for (int e = 0; e < 4 && f0 + e < lim; ++e) dst[e] = src[e];
        }
    }
}

__global__ void __launch_bounds__(256)
    wloss_exposure_reduce_kernel(const float *__restrict__ partials, int64_t tiles, float *__restrict__ grad_exposure) {
    __shared__ double sa[kTerms][256];
    // sum_records<kTerms>, written out: through the function this kernel compiles to other address arithmetic in front of
    // its loop, and the one timing it can be held to did not place it inside the parent's spread (docs/lab_notes/loss_shared_text.md)
    double a[kTerms];
#pragma unroll
    for (int k = 0; k < kTerms; ++k) a[k] = 0.0;
    for (int64_t i = threadIdx.x; i < tiles; i += 256)
#pragma unroll
        for (int k = 0; k < kTerms; ++k) a[k] += (double)partials[i * kTerms + k];
#pragma unroll
    for (int k = 0; k < kTerms; ++k) sa[k][threadIdx.x] = a[k];
    __syncthreads();
    for (int half = 128; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half)
#pragma unroll
            for (int k = 0; k < kTerms; ++k) sa[k][threadIdx.x] += sa[k][threadIdx.x + half];
        __syncthreads();
    }
    if (threadIdx.x < kTerms) grad_exposure[threadIdx.x] = (float)sa[threadIdx.x][0];
}

__global__ void __launch_bounds__(64) wloss_weight_sum_kernel(float *__restrict__ loss_out, float n) {
    if (threadIdx.x == 0) loss_out[3] = n;
}

}  // namespace

hipError_t launch_loss_weight_sum(int32_t rows, int32_t cols, float *loss_out, hipStream_t s) {
    wloss_weight_sum_kernel<<<1, 64, 0, s>>>(loss_out, (float)((double)rows * (double)cols));
    return hipGetLastError();
}

hipError_t launch_photometric_loss_weighted(const LossImages &im, const LossWeights &wt, float lambda, float *loss_out, char *ws,
                                            const plan::LossWeightedCarve &c, hipStream_t s) {
    const Taps taps = window_taps();
    const LossLaunch l = loss_launch(im, ws, c.base);
    float *sums = reinterpret_cast<float *>(ws + c.sums), *scale = reinterpret_cast<float *>(ws + c.scale);
    float *partials = (im.grad && wt.grad_exposure) ? reinterpret_cast<float *>(ws + c.exposure) : nullptr;
    hipError_t e = hipSuccess;
#define GSX_WLOSS_MAPS(G, X)                                                                                                   \
    wloss_maps_kernel<G, X><<<l.tiles, NT, 0, s>>>(im.image, im.image_stride, im.target, im.target_stride, wt.weight,          \
                                                   wt.weight_stride, wt.exposure, im.rows, im.cols, taps, l.mu, l.mp, l.mq,     \
                                                   l.map_stride, sums, l.tiles_c, l.vx, l.vy)
    if (l.run & 1) {
        if (im.grad && wt.exposure) GSX_WLOSS_MAPS(true, true);
        else if (im.grad) GSX_WLOSS_MAPS(true, false);
        else if (wt.exposure) GSX_WLOSS_MAPS(false, true);
        else GSX_WLOSS_MAPS(false, false);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
#undef GSX_WLOSS_MAPS
    if (l.run & 2) {
        wloss_reduce_kernel<<<1, 256, 0, s>>>(sums, c.base.tiles, lambda, loss_out, scale);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (im.grad && (l.run & 4)) {
        if (wt.exposure)
            wloss_grad_kernel<true><<<l.tiles, NT, 0, s>>>(im.image, im.image_stride, im.target, im.target_stride, wt.weight,
                                                           wt.weight_stride, wt.exposure, im.grad, im.grad_stride, im.rows,
                                                           im.cols, taps, scale, l.mu, l.mp, l.mq, l.map_stride, partials,
                                                           l.tiles_c, l.vg);
        else
            wloss_grad_kernel<false><<<l.tiles, NT, 0, s>>>(im.image, im.image_stride, im.target, im.target_stride, wt.weight,
                                                            wt.weight_stride, wt.exposure, im.grad, im.grad_stride, im.rows,
                                                            im.cols, taps, scale, l.mu, l.mp, l.mq, l.map_stride, partials,
                                                            l.tiles_c, l.vg);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if (partials) {
            wloss_exposure_reduce_kernel<<<1, 256, 0, s>>>(partials, c.base.tiles, wt.grad_exposure);
            e = hipGetLastError();
        }
    }
    return e;
}

}  // namespace gsx
