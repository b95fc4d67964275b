// The photometric loss of a splat fit, value and dL/dframe in one call (gsx_photometric_loss, include/gsx.h):
//   loss = (1 - lambda) mean|x - y| + lambda (1 - mean SSIM(x, y)),  11 x 11 Gaussian window, sigma 1.5, zero padding 5,
// over the rows x cols region at the origin of two channel-interleaved (.., .., 3) images, as if both were cropped to it.
//
// BUILD EXTENSION -- the reference renders and stops; the objective is the published one of 3D Gaussian Splatting
// (Kerbl et al. 2023) with the SSIM of Wang et al. 2004.  Parity is pinned to the float64 restatement of the formula
// (tests/photometric_loss_restatement.py) within 12 x the error torch's own float32 evaluation has against it.
//
// Three kernels, no atomics, every sum in a fixed order (same inputs, same bits):
//   loss_maps_kernel    one workgroup per 32 x 32 tile: both images' tile + 5-pixel halo through LDS (loaded as the
//                       contiguous 3 (32 + 10) floats of a row, 16 bytes at a time where base and stride allow, split
//                       into channel planes in LDS, zero outside the region), then per channel the five quantities
//                       x, y, xx, xy, yy filtered along the row into LDS and along the column into registers; m, |x - y|
//                       and -- with a gradient -- w Dmu, w Dp, w Dq, which leave through LDS as whole interleaved rows;
//                       one (sum m, sum |x - y|) pair per workgroup
//   loss_reduce_kernel  one workgroup: the pairs summed in double, loss_out = (loss, l1, ssim)
//   loss_grad_kernel    the same tiling: each of the three maps staged with its halo (zero outside the region, which is
//                       what makes the zero-padded filter its own adjoint), filtered, combined with x, y and the L1 sign
// Compiled with -ffp-contract=off; the filter taps are explicit fmaf chains.
// The tiling constants, Taps, stage_tile and block_sum are gsx_loss_device.h's, shared with gsx_loss_weighted.hip.
#include "gsx_loss_device.h"

namespace gsx {
namespace {

template <bool GRAD>
__global__ void __launch_bounds__(NT)
    loss_maps_kernel(const float *__restrict__ image, int64_t image_stride, const float *__restrict__ target,
                     int64_t target_stride, int32_t R, int32_t C, Taps taps, float w, float *__restrict__ map_mu,
                     float *__restrict__ map_p, float *__restrict__ map_q, int64_t map_stride, float2 *__restrict__ partials,
                     uint32_t tiles_c, bool vec_x, bool vec_y) {
    __shared__ __attribute__((aligned(16))) float lds[kMapsLds];
    float *px = lds, *py = lds + 3 * kPlane, *hp = lds + 6 * kPlane;
    const uint32_t by = blockIdx.x / tiles_c, bx = blockIdx.x % tiles_c;
    const int64_t r0 = (int64_t)by * T, c0 = (int64_t)bx * T, cf0 = 3 * c0;
    stage_tile(image, image_stride, R, C, r0, cf0, px, vec_x);
    stage_tile(target, target_stride, R, C, r0, cf0, py, vec_y);
    __syncthreads();
    const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
    const int tr = threadIdx.x / T, tc = threadIdx.x % T;
    float sum_m = 0.0f, sum_d = 0.0f;
    float o[3][3][PX];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float *cx = px + ch * kPlane, *cy = py + ch * kPlane;
        for (int idx = threadIdx.x; idx < S * T; idx += NT) {
            const int i = idx / T, c = idx % T;
            float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f, a4 = 0.0f;
#pragma unroll
            for (int k = 0; k < kTaps; ++k) {
                const float x = cx[i * S + c + k], y = cy[i * S + c + k], g = taps.g[k];
                a0 = fmaf(g, x, a0);
                a1 = fmaf(g, y, a1);
                a2 = fmaf(g, x * x, a2);
                a3 = fmaf(g, x * y, a3);
                a4 = fmaf(g, y * y, a4);
            }
            hp[0 * S * T + idx] = a0;
            hp[1 * S * T + idx] = a1;
            hp[2 * S * T + idx] = a2;
            hp[3 * S * T + idx] = a3;
            hp[4 * S * T + idx] = a4;
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < PX; ++m) {
            const int r = tr + (NT / T) * m;
            float mu1 = 0.0f, mu2 = 0.0f, p = 0.0f, q = 0.0f, rr = 0.0f;
#pragma unroll
            for (int k = 0; k < kTaps; ++k) {
                const float g = taps.g[k];
                const int at = (r + k) * T + tc;
                mu1 = fmaf(g, hp[0 * S * T + at], mu1);
                mu2 = fmaf(g, hp[1 * S * T + at], mu2);
                p = fmaf(g, hp[2 * S * T + at], p);
                q = fmaf(g, hp[3 * S * T + at], q);
                rr = fmaf(g, hp[4 * S * T + at], rr);
            }
            const bool inside = r0 + r < R && c0 + tc < C;
            const float x = cx[(r + H) * S + tc + H], y = cy[(r + H) * S + tc + H];
            const float mu1sq = mu1 * mu1, mu2sq = mu2 * mu2, mu12 = mu1 * mu2;
            const float s1 = p - mu1sq, s2 = rr - mu2sq, s12 = q - mu12;
            const float A1 = 2.0f * mu12 + C1, A2 = 2.0f * s12 + C2;
            const float B1 = mu1sq + mu2sq + C1, B2 = s1 + s2 + C2;
            const float B12 = B1 * B2, A12 = A1 * A2;
            const float mval = A12 / B12;
            if (inside) {
                sum_m += mval;
                sum_d += fabsf(x - y);
            }
            if (GRAD) {
                const float dmu = 2.0f * mu2 * (A2 - A1) / B12 - 2.0f * mu1 * A12 * (B2 - B1) / (B12 * B12);
                const float dp = -A12 / (B12 * B2);
                const float dq = 2.0f * A1 / B12;
                o[0][ch][m] = inside ? w * dmu : 0.0f;
                o[1][ch][m] = inside ? w * dp : 0.0f;
                o[2][ch][m] = inside ? w * dq : 0.0f;
            }
        }
        __syncthreads();     // the next channel overwrites hp
    }
    float *red = hp;
    const float tot_m = block_sum(sum_m, red), tot_d = block_sum(sum_d, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = make_float2(tot_m, tot_d);
    if (!GRAD) return;
    // the three maps leave as whole interleaved rows: obuf[map][r][3 c + ch] over the staging area, which nobody reads any more
    float *obuf = lds;
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
#pragma unroll
            for (int m = 0; m < PX; ++m) obuf[(k * T + tr + (NT / T) * m) * kRowFloats + 3 * tc + ch] = o[k][ch][m];
    __syncthreads();
    const int64_t lim = 3 * (int64_t)C;
    for (int idx = threadIdx.x; idx < 3 * T * kRowQuads; idx += NT) {
        const int k = idx / (T * kRowQuads), rem = idx % (T * kRowQuads), r = rem / kRowQuads, q = rem % kRowQuads;
        const int64_t row = r0 + r, f0 = cf0 + 4 * q;
        if (row >= R || f0 >= lim) continue;
        float *dst = (k == 0 ? map_mu : (k == 1 ? map_p : map_q)) + row * map_stride + f0;   // 16-byte aligned: map_stride % 4 == 0
        const float *src = obuf + (k * T + r) * kRowFloats + 4 * q;
        if (f0 + 4 <= lim) {
            *reinterpret_cast<float4 *>(dst) = *reinterpret_cast<const float4 *>(src);
        } else {
            for (int e = 0; f0 + e < lim; ++e) dst[e] = src[e];
        }
    }
}

__global__ void __launch_bounds__(256)
    loss_reduce_kernel(const float2 *__restrict__ partials, int64_t tiles, double n, float lambda, float *__restrict__ loss_out) {
    __shared__ double sa[256], sb[256];
    double a = 0.0, b = 0.0;
    for (int64_t i = threadIdx.x; i < tiles; i += 256) {
        const float2 p = partials[i];
        a += (double)p.x;
        b += (double)p.y;
    }
    sa[threadIdx.x] = a;
    sb[threadIdx.x] = b;
    __syncthreads();
    for (int half = 128; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) {
            sa[threadIdx.x] += sa[threadIdx.x + half];
            sb[threadIdx.x] += sb[threadIdx.x + half];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double ssim = sa[0] / n, l1 = sb[0] / n, lam = (double)lambda;
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
    __shared__ __attribute__((aligned(16))) float lds[kGradLds];
    float *planes = lds, *hp = lds + 3 * kPlane;
    const uint32_t by = blockIdx.x / tiles_c, bx = blockIdx.x % tiles_c;
    const int64_t r0 = (int64_t)by * T, c0 = (int64_t)bx * T, cf0 = 3 * c0;
    const int tr = threadIdx.x / T, tc = threadIdx.x % T;
    float F[3][3][PX];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        stage_tile(k == 0 ? map_mu : (k == 1 ? map_p : map_q), map_stride, R, C, r0, cf0, planes, true);
        __syncthreads();
        for (int idx = threadIdx.x; idx < 3 * S * T; idx += NT) {
            const int ch = idx / (S * T), rem = idx % (S * T), i = rem / T, c = rem % T;
            float a = 0.0f;
#pragma unroll
            for (int t = 0; t < kTaps; ++t) a = fmaf(taps.g[t], planes[ch * kPlane + i * S + c + t], a);
            hp[idx] = a;
        }
        __syncthreads();
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
#pragma unroll
            for (int m = 0; m < PX; ++m) {
                const int r = tr + (NT / T) * m;
                float a = 0.0f;
#pragma unroll
                for (int t = 0; t < kTaps; ++t) a = fmaf(taps.g[t], hp[ch * S * T + (r + t) * T + tc], a);
                F[k][ch][m] = a;
            }
        __syncthreads();     // the next map overwrites planes and hp
    }
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
    const bool vx = rows_aligned(im.image, im.image_stride), vy = rows_aligned(im.target, im.target_stride);
    float2 *partials = reinterpret_cast<float2 *>(ws + c.partials);
    float *mu = im.grad ? reinterpret_cast<float *>(ws + c.maps[0]) : nullptr;
    float *mp = im.grad ? reinterpret_cast<float *>(ws + c.maps[1]) : nullptr;
    float *mq = im.grad ? reinterpret_cast<float *>(ws + c.maps[2]) : nullptr;
    const unsigned tiles = (unsigned)c.tiles, tiles_c = (unsigned)c.tiles_c;
    // test library only: which of the three launches run (tools/bench_loss.py times them one by one)
    const int run = knob("GSX_LOSS_KERNELS", 7);
    hipError_t e = hipSuccess;
    if (run & 1) {
        if (im.grad)
            loss_maps_kernel<true><<<tiles, NT, 0, s>>>(im.image, im.image_stride, im.target, im.target_stride, im.rows, im.cols,
                                                        taps, w, mu, mp, mq, c.map_stride, partials, tiles_c, vx, vy);
        else
            loss_maps_kernel<false><<<tiles, NT, 0, s>>>(im.image, im.image_stride, im.target, im.target_stride, im.rows, im.cols,
                                                         taps, w, mu, mp, mq, c.map_stride, partials, tiles_c, vx, vy);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (run & 2) {
        loss_reduce_kernel<<<1, 256, 0, s>>>(partials, c.tiles, n, lambda, loss_out);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (im.grad && (run & 4)) {
        loss_grad_kernel<<<tiles, NT, 0, s>>>(im.image, im.image_stride, im.target, im.target_stride, im.grad, im.grad_stride,
                                              im.rows, im.cols, taps, l1_weight, mu, mp, mq, c.map_stride, tiles_c, vx, vy,
                                              rows_aligned(im.grad, im.grad_stride));
        e = hipGetLastError();
    }
    return e;
}

}  // namespace gsx
