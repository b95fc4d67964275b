// What the kernels of gsx_loss.hip (gsx_photometric_loss) and gsx_loss_weighted.hip (gsx_photometric_loss_weighted) share:
// the tiling constants, the window taps, the staging of a tile + halo into channel planes in LDS, the fixed-order
// workgroup sum, the reduce kernels' double tree and what the launchers read off the carve.  The two big passages of the
// tile kernels are text, not functions: gsx_loss_maps.inc and gsx_loss_grad_filter.inc.
// Everything sits in an anonymous namespace: each translation unit compiles its own copy, inlined.
#pragma once

#include "gsx_internal.h"

namespace gsx {
namespace {

constexpr int T = plan::kLossTile, H = plan::kLossHalo, S = T + 2 * H;   // tile edge, halo, staged edge (42)
constexpr int kTaps = 2 * H + 1;
constexpr int NT = 512;                 // threads per workgroup
constexpr int PX = T * T / NT;          // output pixels per thread: (tid / T + (NT / T) m, tid % T)
constexpr int kRowFloats = 3 * T;       // an interleaved tile row
constexpr int kRowQuads = kRowFloats / 4;
constexpr int kPlane = S * S;
static_assert(T == 32 && (NT % T) == 0 && PX * NT == T * T && (kRowFloats % 4) == 0, "the index arithmetic below");

struct Taps {
    float g[kTaps];
};

// The tile at (r0, c0 = cf0 / 3) with its halo, out of an image of R x C pixels with `stride` floats per row, into the
// three channel planes planes[ch][S][S]; zero outside the image.  A staged row is the 3 S contiguous floats from cf0 - 15.
// vec: rows start 16-byte aligned (base and stride); the row is then read as the 32 float4 from cf0 - 16 (cf0 is a
// multiple of 96), a float4 that straddles the row's end element by element.
__device__ __forceinline__ void stage_tile(const float *__restrict__ img, int64_t stride, int32_t R, int32_t C, int64_t r0,
                                           int64_t cf0, float *__restrict__ planes, bool vec) {
    const int64_t lim = 3 * (int64_t)C;
    if (vec) {
        for (int idx = threadIdx.x; idx < S * 32; idx += NT) {
            const int i = idx >> 5, q = idx & 31;
            const int64_t rr = r0 - H + i, f0 = cf0 - 16 + 4 * q;
            float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (rr >= 0 && rr < R) {
                const float *row = img + rr * stride;
                if (f0 >= 0 && f0 + 4 <= lim) {
                    const float4 t = *reinterpret_cast<const float4 *>(row + f0);
                    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (f0 + e >= 0 && f0 + e < lim) v[e] = row[f0 + e];
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int j = 4 * q - 1 + e;
                if (j >= 0 && j < 3 * S) planes[(j % 3) * kPlane + i * S + j / 3] = v[e];
            }
        }
    } else {
        for (int idx = threadIdx.x; idx < S * 3 * S; idx += NT) {
            const int i = idx / (3 * S), j = idx % (3 * S);
            const int64_t rr = r0 - H + i, f = cf0 - 3 * H + j;
            float v = 0.0f;
            if (rr >= 0 && rr < R && f >= 0 && f < lim) v = img[rr * stride + f];
            planes[(j % 3) * kPlane + i * S + j / 3] = v;
        }
    }
}

// Sum over the workgroup in a fixed order: down the lanes of a wave, then the waves in turn.  Result in thread 0.
__device__ __forceinline__ float block_sum(float v, float *red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = 0.0f;
    if (threadIdx.x == 0)
        for (int k = 0; k < NT / 64; ++k) s += red[k];
    __syncthreads();
    return s;
}

// The reduce kernels' sum (one workgroup of 256 threads): `tiles` records of K floats, the K columns side by side, in
// double and in a fixed order -- strided over the threads, then a halving tree.  Column k's sum is sa[k][0], for every thread.
template <int K>
__device__ __forceinline__ void sum_records(const float *__restrict__ rec, int64_t tiles, double (&sa)[K][256]) {
    double a[K];
#pragma unroll
    for (int k = 0; k < K; ++k) a[k] = 0.0;
    for (int64_t i = threadIdx.x; i < tiles; i += 256)
#pragma unroll
        for (int k = 0; k < K; ++k) a[k] += (double)rec[i * K + k];
#pragma unroll
    for (int k = 0; k < K; ++k) sa[k][threadIdx.x] = a[k];
    __syncthreads();
    for (int half = 128; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half)
#pragma unroll
            for (int k = 0; k < K; ++k) sa[k][threadIdx.x] += sa[k][threadIdx.x + half];
        __syncthreads();
    }
}

constexpr int kMapsLds = 6 * kPlane + 5 * S * T;    // x, y planes of three channels + five row-filtered planes: 69 216 bytes
constexpr int kGradLds = 3 * kPlane + 3 * S * T;    // one map's three planes + their row-filtered planes:       37 296 bytes
static_assert(3 * T * kRowFloats <= 6 * kPlane && 3 * T * kRowFloats <= kGradLds, "the outgoing rows reuse the staging area");
static_assert(kMapsLds * sizeof(float) <= 80 * 1024, "two workgroups per CU");

inline bool rows_aligned(const void *base, int64_t stride) {
    return (reinterpret_cast<uintptr_t>(base) & 15u) == 0 && (stride & 3) == 0;
}

// What both launchers read off the images and the plain carve (the weighted carve starts with it) and hand to their
// kernels as plain arguments.
struct LossLaunch {
    float *mu, *mp, *mq;        // the three maps in the workspace; nullptr without a gradient
    int64_t map_stride;
    unsigned tiles, tiles_c;    // workgroups of a tile kernel; tiles per tile row
    bool vx, vy, vg;            // rows_aligned: image, target, grad
    int run;                    // test library only: which launches run, GSX_LOSS_KERNELS = 1 maps | 2 reduce | 4 gradient
                                // (tools/bench_loss.py times them one by one)
};

inline LossLaunch loss_launch(const LossImages &im, char *ws, const plan::LossCarve &c) {
    LossLaunch l{};
    if (im.grad) {
        l.mu = reinterpret_cast<float *>(ws + c.maps[0]);
        l.mp = reinterpret_cast<float *>(ws + c.maps[1]);
        l.mq = reinterpret_cast<float *>(ws + c.maps[2]);
    }
    l.map_stride = c.map_stride;
    l.tiles = (unsigned)c.tiles;
    l.tiles_c = (unsigned)c.tiles_c;
    l.vx = rows_aligned(im.image, im.image_stride);
    l.vy = rows_aligned(im.target, im.target_stride);
    l.vg = rows_aligned(im.grad, im.grad_stride);
    l.run = knob("GSX_LOSS_KERNELS", 7);
    return l;
}

// g[i] = exp(-(i - 5)^2 / (2 1.5^2)) / sum, formed in double, rounded once.
inline Taps window_taps() {
    Taps taps;
    double g[kTaps], sum = 0.0;
    for (int i = 0; i < kTaps; ++i) {
        g[i] = exp(-(double)((i - H) * (i - H)) / (2.0 * 1.5 * 1.5));
        sum += g[i];
    }
    for (int i = 0; i < kTaps; ++i) taps.g[i] = (float)(g[i] / sum);
    return taps;
}

}  // namespace
}  // namespace gsx
