// gsx_mcmc_regularize / gsx_mcmc_perturb / gsx_mcmc_plan / gsx_mcmc_apply: fixed-budget densification, the relocation and
// the position noise of 3DGS-MCMC (Kheradmand et al. 2024), over every array of a Gaussian container and the optimiser's
// moments.
//
// BUILD EXTENSION -- the reference renders and stops.  The formulas, the integer rule of the plan and the float32 operation
// order of the two per-step kernels are the contract of include/gsx.h and are restated in tests/mcmc_restatement.py; the
// library is built with -ffp-contract=off and correctly rounded divide and sqrt.
//
// Regularize and perturb: pure streams, one launch each, no LDS.  A thread owns a few consecutive rows, so that every
// array of the row -- 3, 4 or 1 floats wide -- is read and written as whole vectors when its base is 16-byte aligned:
// four rows in regularize (four rows of a 3-wide array are three 16-byte vectors), two in perturb (8-byte vectors, the
// quaternions 16-byte).  Perturb carries 17 floats and two expf, a sqrt and four divides per row: at four rows per thread
// a 1M-row call was 3900 waves, half of what the device holds at once, and streamed at 3.5 TB/s; at two rows it is 7800
// waves of 56 VGPRs and streams at 5.5 TB/s, beside gsx_adam_step's 5.9 (tools/bench_mcmc.py).  Rows behind the last
// whole group, and every row of a call with an unaligned base, go float by float through the same arithmetic.
//
// Plan: a workgroup weighs kMcmcScanRows = 1024 rows (four per thread), leaves their weights, zeroes their counts and
// leaves every row's exclusive prefix INSIDE the block (32 bits are enough there) with the block's sum; one workgroup scans
// the block sums in 64 bits and writes the header; then one thread per output row draws: a binary search over the block
// sums, then over the prefixes of that block's rows, and one integer atomic on the source's count.  Three launches and no
// look-back chain, as in gsx_density.hip.
//
// Apply: a gather-stream.  A workgroup owns kMcmcRows = 256 consecutive OUTPUT rows, one contiguous run in every group.
// Per row the source, whether it moved (N > 1) and, for a moved row, its new opacity logit and its scale factor -- the
// published relocation, in double -- are left in LDS once; then every group's run is walked front to back as in
// density_apply_kernel: 16-byte stores from the run's first 16-byte boundary on, and one 16-byte load per quad where the
// width is a multiple of four floats and both sides are aligned.  The group descriptors are read from the
// kernel-argument segment with scalar loads.
#include "gsx_internal.h"

namespace gsx {
namespace {

using plan::kMcmcScanRows;

constexpr int kThreads = 256, kScanPer = kMcmcScanRows / kThreads, kRowsPer = 4, kPerturbRows = 2;
static_assert(kScanPer == 4 && kMcmcRows == kThreads, "four rows per thread in the scan, one in the apply");

__device__ __forceinline__ bool finite32(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// ---------------------------------------------------------------------------------------------------- regularize
__device__ __forceinline__ float reg_opacity(float g, float o, float coef) {
    const float sg = 1.0f / (1.0f + expf(-o));
    return g + coef * (sg * (1.0f - sg));
}
__device__ __forceinline__ float reg_scale(float g, float s, float coef) {
    return s > 0.0f ? g + coef : (s < 0.0f ? g - coef : g);
}

__global__ void __launch_bounds__(kThreads) mcmc_regularize_kernel(const McmcRegularizeArgs k) {
    const int64_t r0 = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * kRowsPer;
    if (r0 >= k.n) return;
    if (k.vec && r0 + kRowsPer <= k.n) {
        if (k.grad_opacity) {
            const float4 o = *reinterpret_cast<const float4 *>(k.opacity + r0);
            float4 g = *reinterpret_cast<float4 *>(k.grad_opacity + r0);
            g.x = reg_opacity(g.x, o.x, k.coef_opacity);
            g.y = reg_opacity(g.y, o.y, k.coef_opacity);
            g.z = reg_opacity(g.z, o.z, k.coef_opacity);
            g.w = reg_opacity(g.w, o.w, k.coef_opacity);
            *reinterpret_cast<float4 *>(k.grad_opacity + r0) = g;
        }
        if (k.grad_scales) {
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const float4 s = reinterpret_cast<const float4 *>(k.scales + 3 * r0)[q];
                float4 g = reinterpret_cast<float4 *>(k.grad_scales + 3 * r0)[q];
                g.x = reg_scale(g.x, s.x, k.coef_scale);
                g.y = reg_scale(g.y, s.y, k.coef_scale);
                g.z = reg_scale(g.z, s.z, k.coef_scale);
                g.w = reg_scale(g.w, s.w, k.coef_scale);
                reinterpret_cast<float4 *>(k.grad_scales + 3 * r0)[q] = g;
            }
        }
        return;
    }
    const int64_t left = k.n - r0;
    const int rows = left < kRowsPer ? (int)left : kRowsPer;
    for (int j = 0; j < rows; ++j) {
        const int64_t r = r0 + j;
        if (k.grad_opacity) k.grad_opacity[r] = reg_opacity(k.grad_opacity[r], k.opacity[r], k.coef_opacity);
        if (k.grad_scales)
            for (int c = 0; c < 3; ++c) k.grad_scales[3 * r + c] = reg_scale(k.grad_scales[3 * r + c], k.scales[3 * r + c], k.coef_scale);
    }
}

// ---------------------------------------------------------------------------------------------------- perturb
// One row, in the operation order of include/gsx.h (gsx_mcmc_perturb); p is left alone when a component of delta is not finite.
__device__ __forceinline__ void perturb_row(float *p, const float *s, const float *q, float o, const float *e, float rate,
                                            float gate_k, float gate_x0) {
    const float sg = 1.0f / (1.0f + expf(-o));
    const float gate = 1.0f / (1.0f + expf(-(gate_k * ((1.0f - sg) - gate_x0))));
    const float nrm = sqrtf(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    const float w = q[0] / nrm, x = q[1] / nrm, y = q[2] / nrm, z = q[3] / nrm;
    float R[3][3];
    R[0][0] = 1.0f - 2.0f * (y * y + z * z);
    R[0][1] = 2.0f * (x * y - w * z);
    R[0][2] = 2.0f * (x * z + w * y);
    R[1][0] = 2.0f * (x * y + w * z);
    R[1][1] = 1.0f - 2.0f * (x * x + z * z);
    R[1][2] = 2.0f * (y * z - w * x);
    R[2][0] = 2.0f * (x * z - w * y);
    R[2][1] = 2.0f * (y * z + w * x);
    R[2][2] = 1.0f - 2.0f * (x * x + y * y);
    float v[3], d[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = (s[c] * s[c]) * ((R[0][c] * e[0] + R[1][c] * e[1]) + R[2][c] * e[2]);
    const float f = rate * gate;
#pragma unroll
    for (int c = 0; c < 3; ++c) d[c] = f * ((R[c][0] * v[0] + R[c][1] * v[1]) + R[c][2] * v[2]);
    if (finite32(d[0]) && finite32(d[1]) && finite32(d[2])) {
        p[0] = p[0] + d[0];
        p[1] = p[1] + d[1];
        p[2] = p[2] + d[2];
    }
}

// COUNT consecutive floats from a 16-byte (ROWS == 4) or 8-byte (ROWS == 2) aligned address, as whole vectors.
template <int ROWS, int COUNT>
__device__ __forceinline__ void load_run(const float *__restrict__ src, float *out) {
    if (ROWS == 4) {
#pragma unroll
        for (int i = 0; i < COUNT / 4; ++i) {
            const float4 v = reinterpret_cast<const float4 *>(src)[i];
            out[4 * i] = v.x; out[4 * i + 1] = v.y; out[4 * i + 2] = v.z; out[4 * i + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < COUNT / 2; ++i) {
            const float2 v = reinterpret_cast<const float2 *>(src)[i];
            out[2 * i] = v.x; out[2 * i + 1] = v.y;
        }
    }
}

// A thread owns ROWS consecutive rows (kPerturbRows in the launch below).
template <int ROWS>
__global__ void __launch_bounds__(kThreads) mcmc_perturb_kernel(const McmcPerturbArgs k) {
    const int64_t r0 = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * ROWS;
    if (r0 >= k.n) return;
    if (k.vec && r0 + ROWS <= k.n) {
        float p[3 * ROWS], s[3 * ROWS], e[3 * ROWS], q[4 * ROWS], o[ROWS];
        load_run<ROWS, 3 * ROWS>(k.points + 3 * r0, p);
        load_run<ROWS, 3 * ROWS>(k.scales + 3 * r0, s);
        load_run<ROWS, 3 * ROWS>(k.noise + 3 * r0, e);
        load_run<4, 4 * ROWS>(k.quats + 4 * r0, q);
        load_run<ROWS, ROWS>(k.opacity + r0, o);
#pragma unroll
        for (int j = 0; j < ROWS; ++j) perturb_row(p + 3 * j, s + 3 * j, q + 4 * j, o[j], e + 3 * j, k.rate, k.gate_k, k.gate_x0);
        if (ROWS == 4) {
            float4 *out = reinterpret_cast<float4 *>(k.points + 3 * r0);
#pragma unroll
            for (int i = 0; i < 3 * ROWS / 4; ++i) out[i] = make_float4(p[4 * i], p[4 * i + 1], p[4 * i + 2], p[4 * i + 3]);
        } else {
            float2 *out = reinterpret_cast<float2 *>(k.points + 3 * r0);
#pragma unroll
            for (int i = 0; i < 3 * ROWS / 2; ++i) out[i] = make_float2(p[2 * i], p[2 * i + 1]);
        }
        return;
    }
    const int64_t left = k.n - r0;
    const int rows = left < ROWS ? (int)left : ROWS;
    for (int j = 0; j < rows; ++j) {
        const int64_t r = r0 + j;
        float p[3] = {k.points[3 * r], k.points[3 * r + 1], k.points[3 * r + 2]};
        const float s[3] = {k.scales[3 * r], k.scales[3 * r + 1], k.scales[3 * r + 2]};
        const float e[3] = {k.noise[3 * r], k.noise[3 * r + 1], k.noise[3 * r + 2]};
        const float q[4] = {k.quats[4 * r], k.quats[4 * r + 1], k.quats[4 * r + 2], k.quats[4 * r + 3]};
        perturb_row(p, s, q, k.opacity[r], e, k.rate, k.gate_k, k.gate_x0);
        k.points[3 * r] = p[0];
        k.points[3 * r + 1] = p[1];
        k.points[3 * r + 2] = p[2];
    }
}

// ---------------------------------------------------------------------------------------------------- plan
// Exclusive scan of one 64-bit value per thread over the 256 threads of the workgroup; total = the sum.
__device__ __forceinline__ uint64_t block_exclusive64(uint64_t v, uint64_t *lds, uint64_t &total) {
    const int t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
#pragma unroll
    for (int s = 1; s < kThreads; s <<= 1) {
        const uint64_t add = t >= s ? lds[t - s] : 0u;
        __syncthreads();
        lds[t] += add;
        __syncthreads();
    }
    total = lds[kThreads - 1];
    const uint64_t incl = lds[t];
    __syncthreads();
    return incl - v;
}

// Per 1024 rows: the weights, zeros in count, the rows' exclusive prefix inside the block, the block's sum and tallies.
__global__ void __launch_bounds__(kThreads)
    mcmc_weights_kernel(const float *__restrict__ opacity, int64_t n, float dead_logit, uint32_t *__restrict__ weights,
                        uint32_t *__restrict__ count, uint32_t *__restrict__ prefix, uint64_t *__restrict__ bsum,
                        uint32_t *__restrict__ btally) {
    __shared__ uint64_t lds[kThreads];
    const int64_t r0 = (int64_t)blockIdx.x * kMcmcScanRows + threadIdx.x * kScanPer;
    uint32_t w[kScanPer];
    uint64_t sum = 0u, tally = 0u;          // tally: dead rows | rows of non-zero weight << 32
#pragma unroll
    for (int j = 0; j < kScanPer; ++j) {
        w[j] = 0u;
        if (r0 + j < n) {
            const float o = opacity[r0 + j];
            const bool dead = o <= dead_logit;
            if (!dead && finite32(o)) {
                const double v = rint(4194304.0 * (1.0 / (1.0 + exp(-(double)o))));
                w[j] = v < 1.0 ? 1u : (uint32_t)v;
            }
            weights[r0 + j] = w[j];
            count[r0 + j] = 0u;
            tally += (dead ? 1u : 0u) + (w[j] != 0u ? (uint64_t)1 << 32 : 0u);
            sum += w[j];
        }
    }
    uint64_t total, total2;
    uint32_t at = (uint32_t)block_exclusive64(sum, lds, total);      // < 1024 * 2^22: the last row's prefix fits 32 bits
    (void)block_exclusive64(tally, lds, total2);
#pragma unroll
    for (int j = 0; j < kScanPer; ++j) {
        if (r0 + j < n) prefix[r0 + j] = at;
        at += w[j];
    }
    if (threadIdx.x == 0) {
        bsum[blockIdx.x] = total;
        btally[2 * blockIdx.x] = (uint32_t)total2;
        btally[2 * blockIdx.x + 1] = (uint32_t)(total2 >> 32);
    }
}

// One workgroup: exclusive scan of the nb block sums in place (bsum[nb] = total), the tallies' totals, the header.
__global__ void __launch_bounds__(kThreads)
    mcmc_blocks_kernel(uint64_t *__restrict__ bsum, const uint32_t *__restrict__ btally, uint32_t nb, char *__restrict__ header) {
    __shared__ uint64_t lds[kThreads];
    uint64_t carry = 0u, dead = 0u, live = 0u;
    for (uint32_t base = 0; base < nb; base += kThreads) {
        const uint32_t i = base + threadIdx.x;
        const uint64_t v = i < nb ? bsum[i] : 0u;
        uint64_t total;
        const uint64_t ex = block_exclusive64(v, lds, total);
        if (i < nb) {
            bsum[i] = carry + ex;
            dead += btally[2 * i];
            live += btally[2 * i + 1];
        }
        carry += total;
    }
    uint64_t n_dead, n_live;
    (void)block_exclusive64(dead, lds, n_dead);
    (void)block_exclusive64(live, lds, n_live);
    if (threadIdx.x == 0) {
        bsum[nb] = carry;
        int64_t *h = reinterpret_cast<int64_t *>(header);
        h[0] = (int64_t)n_dead;
        h[1] = (int64_t)n_live;
        h[2] = (int64_t)carry;
    }
}

// One thread per output row: its source, and one more on the source's count when it is drawn.
__global__ void __launch_bounds__(kThreads)
    mcmc_draw_kernel(const float *__restrict__ opacity, const double *__restrict__ uniforms, const uint32_t *__restrict__ prefix,
                     const uint64_t *__restrict__ bsum, uint32_t nb, int64_t n, int64_t n_out, float dead_logit,
                     int32_t *__restrict__ source, uint32_t *__restrict__ count) {
    const int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (j >= n_out) return;
    const uint64_t total = bsum[nb];
    if (total == 0u) {
        source[j] = (int32_t)(j < n ? j : n - 1);
        return;
    }
    if (j < n && !(opacity[j] <= dead_logit)) {
        source[j] = (int32_t)j;
        return;
    }
    const double x = floor(uniforms[j] * (double)total);
    uint64_t t = x >= 0.0 ? (x < 18446744073709551616.0 ? (uint64_t)x : total) : 0u;     // (a NaN or negative uniform: t = 0)
    t = t < total - 1u ? t : total - 1u;
    uint32_t lo = 0u, hi = nb;                  // the last block with bsum[b] <= t; t < total = bsum[nb], bsum[0] = 0
    while (hi - lo > 1u) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (bsum[mid] <= t) lo = mid; else hi = mid;
    }
    const uint32_t r = (uint32_t)(t - bsum[lo]);
    const int64_t first = (int64_t)lo * kMcmcScanRows, end = first + kMcmcScanRows < n ? first + kMcmcScanRows : n;
    int64_t a = first, b = end;                 // the last row of the block with prefix <= r (prefix[first] = 0)
    while (b - a > 1) {
        const int64_t mid = a + ((b - a) >> 1);
        if (prefix[mid] <= r) a = mid; else b = mid;
    }
    source[j] = (int32_t)a;
    atomicAdd(&count[a], 1u);
}

// ---------------------------------------------------------------------------------------------------- apply
__device__ __forceinline__ float moved_element(const float *__restrict__ src, uint32_t w, int role, const int32_t *srow,
                                               const uint32_t *moved, const float *new_logit, const double *coeff, uint32_t j,
                                               uint32_t kk) {
    if (moved[j]) {
        if (role == GSX_MCMC_ZERO_MOVED) return 0.0f;
        if (role == GSX_MCMC_OPACITY) return new_logit[j];
    }
    const float v = src[(int64_t)srow[j] * (int64_t)w + kk];
    if (moved[j] && role == GSX_MCMC_SCALES) return (float)(coeff[j] * (double)v);
    return v;
}

__global__ void __launch_bounds__(kMcmcRows) mcmc_apply_kernel(const McmcApplyArgs k) {
    __shared__ int32_t srow[kMcmcRows];
    __shared__ uint32_t moved[kMcmcRows];
    __shared__ float new_logit[kMcmcRows];
    __shared__ double coeff[kMcmcRows];
    __shared__ double root[GSX_MCMC_N_MAX];
    const uint32_t tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * kMcmcRows, row = row0 + tid;
    const int64_t left = k.n_out - row0;
    const uint32_t rows = left < (int64_t)kMcmcRows ? (uint32_t)left : (uint32_t)kMcmcRows;
    if (tid < (uint32_t)GSX_MCMC_N_MAX) root[tid] = sqrt((double)(tid + 1u));
    __syncthreads();
    int32_t s = 0;
    uint32_t N = 1u;
    if (tid < rows) {
        const int64_t own = row < k.n ? row : k.n - 1;
        const int64_t got = k.source[row];
        // (a plan is trusted only as far as it stays inside the arrays)
        const bool inside = got >= 0 && got < k.n;
        s = (int32_t)(inside ? got : own);
        const uint32_t c = inside ? k.count[s] : 0u;
        N = c < (uint32_t)GSX_MCMC_N_MAX - 1u ? c + 1u : (uint32_t)GSX_MCMC_N_MAX;
    }
    srow[tid] = s;
    moved[tid] = N > 1u ? 1u : 0u;
    new_logit[tid] = 0.0f;
    coeff[tid] = 1.0;
    if (N > 1u && k.opacity) {
        const double top = 1.0 - 0x1p-24, lowest = (double)k.min_opacity;
        double a = 1.0 / (1.0 + exp(-(double)k.opacity[s]));
        a = a < top ? a : top;
        const double x = -expm1(log1p(-a) / (double)N);
        double D = 0.0;
        for (uint32_t i = 1; i <= N; ++i) {
            double C = 1.0, xp = x, sign = 1.0;
            for (uint32_t kk = 0; kk < i; ++kk) {
                D = D + ((C * sign) * xp) / root[kk];
                C = (C * (double)(i - 1u - kk)) / (double)(kk + 1u);
                xp = xp * x;
                sign = -sign;
            }
        }
        coeff[tid] = a / D;
        double p = x < lowest ? lowest : x;
        p = p > top ? top : p;
        new_logit[tid] = (float)log(p / (1.0 - p));
    }
    __syncthreads();

    for (int gi = 0; gi < k.n_groups; ++gi) {
        const DensityGroupArgs &G = k.group[gi];
        const uint32_t w = (uint32_t)G.width, count = rows * w;
        const int role = G.role;
        const float *src = G.src;
        float *dst = G.dst + row0 * (int64_t)w;
        uint32_t lead = (4u - ((uint32_t)(reinterpret_cast<uintptr_t>(dst) >> 2) & 3u)) & 3u;
        lead = lead < count ? lead : count;
        const uint32_t nvec = (count - lead) / 4u;
        // a width of whole quads between 16-byte aligned sides (the coefficients and their moments: four fifths of a trained
        // scene's bytes): no quad straddles a row, so a quad is one 16-byte load of its source row, or zeros
        if ((w & 3u) == 0u && lead == 0u && (reinterpret_cast<uintptr_t>(src) & 15u) == 0u && role <= GSX_MCMC_ZERO_MOVED) {
            const uint32_t wq = w >> 2;
            for (uint32_t q = tid; q < nvec; q += kMcmcRows) {
                const uint32_t j = q / wq;
                float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (role != GSX_MCMC_ZERO_MOVED || !moved[j])
                    v = reinterpret_cast<const float4 *>(src)[(int64_t)srow[j] * (int64_t)wq + (q - j * wq)];
                reinterpret_cast<float4 *>(dst)[q] = v;
            }
            continue;
        }
        for (uint32_t e = tid; e < lead; e += kMcmcRows) {
            const uint32_t j = e / w;
            dst[e] = moved_element(src, w, role, srow, moved, new_logit, coeff, j, e - j * w);
        }
        for (uint32_t q = tid; q < nvec; q += kMcmcRows) {
            const uint32_t e0 = lead + 4u * q;
            uint32_t j = e0 / w, kk = e0 - j * w;
            float x[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                x[i] = moved_element(src, w, role, srow, moved, new_logit, coeff, j, kk);
                if (++kk == w) { kk = 0u; ++j; }
            }
            *reinterpret_cast<float4 *>(dst + e0) = make_float4(x[0], x[1], x[2], x[3]);
        }
        for (uint32_t e = lead + 4u * nvec + tid; e < count; e += kMcmcRows) {
            const uint32_t j = e / w;
            dst[e] = moved_element(src, w, role, srow, moved, new_logit, coeff, j, e - j * w);
        }
    }
}

}  // namespace

hipError_t launch_mcmc_regularize(const McmcRegularizeArgs &args, hipStream_t s) {
    if (args.n <= 0 || (!args.grad_opacity && !args.grad_scales)) return hipSuccess;
    const int64_t threads = (args.n + kRowsPer - 1) / kRowsPer;
    mcmc_regularize_kernel<<<(unsigned)((threads + kThreads - 1) / kThreads), kThreads, 0, s>>>(args);
    return hipGetLastError();
}

hipError_t launch_mcmc_perturb(const McmcPerturbArgs &args, hipStream_t s) {
    if (args.n <= 0) return hipSuccess;
    const int64_t threads = (args.n + kPerturbRows - 1) / kPerturbRows;
    mcmc_perturb_kernel<kPerturbRows><<<(unsigned)((threads + kThreads - 1) / kThreads), kThreads, 0, s>>>(args);
    return hipGetLastError();
}

hipError_t launch_mcmc_plan(const McmcPlanArgs &a, char *ws, const plan::McmcCarve &c, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    const uint32_t nb = c.scan_blocks;
    uint32_t *prefix = reinterpret_cast<uint32_t *>(ws + c.prefix), *btally = reinterpret_cast<uint32_t *>(ws + c.btally);
    uint64_t *bsum = reinterpret_cast<uint64_t *>(ws + c.bsum);
    mcmc_weights_kernel<<<nb, kThreads, 0, s>>>(a.opacity, a.n, a.dead_logit, a.weights, a.count, prefix, bsum, btally);
    mcmc_blocks_kernel<<<1, kThreads, 0, s>>>(bsum, btally, nb, ws);
    mcmc_draw_kernel<<<(unsigned)((a.n_out + kThreads - 1) / kThreads), kThreads, 0, s>>>(a.opacity, a.uniforms, prefix, bsum, nb, a.n,
                                                                                         a.n_out, a.dead_logit, a.source, a.count);
    return hipGetLastError();
}

hipError_t launch_mcmc_apply(const McmcApplyArgs &args, hipStream_t s) {
    if (args.n <= 0 || args.n_out <= 0) return hipSuccess;
    mcmc_apply_kernel<<<(unsigned)((args.n_out + kMcmcRows - 1) / kMcmcRows), kMcmcRows, 0, s>>>(args);
    return hipGetLastError();
}

}  // namespace gsx
