// gsx_density_accumulate / gsx_density_plan / gsx_density_apply: adaptive density control -- prune, clone, split -- over
// every array of a Gaussian container and the optimiser's moments.
//
// BUILD EXTENSION -- the reference renders and stops; this is the densification of the published 3D Gaussian Splatting
// trainer (Kerbl et al. 2023), with the three differences include/gsx.h states (the statistic's gradient, prune before
// densify, children beside the parent).  The rules, the split formulas and their float32 operation order are the contract
// of include/gsx.h and are restated op for op in tests/density_restatement.py; the library is built with
// -ffp-contract=off and correctly rounded divide and sqrt, so all three calls are reproducible bit for bit from numpy.
//
// Plan: a workgroup classifies kDensityScanRows = 1024 rows (four per thread), leaves their action bytes and the block's
// output-row, pruned and split counts; one workgroup scans the block sums and writes the header; the blocks run again
// and leave every row's first output row.  Three launches and no look-back chain: the fences a chained scan needs cost more
// than the two extra launches save (tools/microbench_lookback.hip).
//
// Apply: a pure gather-stream.  A workgroup owns kDensityRows = 256 consecutive source rows (the block gsx_adam_step and
// block_bounds use); because rows stay in source order with the children beside their parent, the block's output is ONE
// contiguous run of at most 512 rows in every group.  The run's row table -- source row, and continued / clone / child 0 /
// child 1 -- is built once in LDS, as are the six position offsets of every split row; then every group's run is walked
// front to back, with 16-byte stores from the first 16-byte boundary of the run on and float by float before it and
// behind the last whole vector (an element's value does not depend on which path stores it); where the width is a multiple
// of four floats and both runs are 16-byte aligned, a quad is one 16-byte load as well.  The group index is uniform,
// so the descriptors are read from the kernel-argument segment with scalar loads.  Each element of a surviving row is read
// once and written once; nothing is read of a pruned row but its action.
#include "gsx_density_device.h"

namespace gsx {
namespace {

using namespace density;    // kThreads, kScanPer, rows_of, max_nan, block_exclusive, classify, leave_block

__global__ void __launch_bounds__(kThreads)
    density_accumulate_kernel(const float *__restrict__ grad, uint32_t width, int64_t n, float *__restrict__ grad_sum,
                              uint32_t *__restrict__ seen) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const float *g = grad + i * (int64_t)width;
    float sum = g[0] * g[0];
    bool any = (__float_as_uint(g[0]) & 0x7fffffffu) != 0u;
    for (uint32_t k = 1; k < width; ++k) {
        const float x = g[k];
        sum = sum + x * x;
        any = any || (__float_as_uint(x) & 0x7fffffffu) != 0u;
    }
    if (!any) return;
    grad_sum[i] = grad_sum[i] + sqrtf(sum);
    seen[i] = seen[i] + 1u;
}

// Per 1024 rows: the action bytes (rows behind n: PRUNE, counted nowhere), and the block's output rows, pruned and split rows.
__global__ void __launch_bounds__(kThreads)
    density_classify_kernel(const float *__restrict__ grad_sum, const uint32_t *__restrict__ seen,
                            const float *__restrict__ scales, const float *__restrict__ opacity_logit, int64_t n,
                            const GsxDensityRules rules, uint32_t *__restrict__ action4, uint32_t *__restrict__ bsum,
                            uint32_t *__restrict__ bpruned, uint32_t *__restrict__ bsplit) {
    __shared__ uint32_t lds[kThreads];
    const int64_t r0 = (int64_t)blockIdx.x * kDensityScanRows + threadIdx.x * kScanPer;
    uint32_t word = 0u, out = 0u, tally = 0u;       // tally: pruned | split << 16 (each at most 1024 in a block)
#pragma unroll
    for (int k = 0; k < kScanPer; ++k) {
        uint32_t a = kDensityPrune;
        if (r0 + k < n) {
            a = classify(grad_sum, seen, scales, opacity_logit, r0 + k, rules);
            out += rows_of(a);
            tally += (a == kDensityPrune ? 1u : 0u) + (a == kDensitySplit ? 0x10000u : 0u);
        }
        word |= a << (8 * k);
    }
    leave_block(word, out, tally, lds, action4, bsum, bpruned, bsplit);
}

// One workgroup: exclusive scan of the nb block sums in place (bsum[nb] = n_out), the pruned and split totals, the header.
__global__ void __launch_bounds__(kThreads)
    density_blocks_kernel(uint32_t *__restrict__ bsum, const uint32_t *__restrict__ bpruned, const uint32_t *__restrict__ bsplit,
                          uint32_t nb, int64_t n, float shrink, char *__restrict__ header) {
    __shared__ uint32_t lds[kThreads];
    uint32_t carry = 0u, pruned = 0u, split = 0u;
    for (uint32_t base = 0; base < nb; base += kThreads) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < nb ? bsum[i] : 0u;
        uint32_t total;
        const uint32_t ex = block_exclusive(v, lds, total);
        if (i < nb) {
            bsum[i] = carry + ex;
            pruned += bpruned[i];
            split += bsplit[i];
        }
        carry += total;
    }
    uint32_t n_pruned, n_split;
    (void)block_exclusive(pruned, lds, n_pruned);
    (void)block_exclusive(split, lds, n_split);
    if (threadIdx.x == 0) {
        bsum[nb] = carry;
        int64_t *h = reinterpret_cast<int64_t *>(header);
        h[0] = n;
        h[1] = (int64_t)carry;
        h[2] = (int64_t)n_pruned;
        h[3] = (int64_t)carry - n + (int64_t)n_pruned - (int64_t)n_split;    // n_out = n - pruned + cloned + split
        h[4] = (int64_t)n_split;
        *reinterpret_cast<float *>(header + kDensityShrinkAt) = shrink;
    }
}

// prefix[i] = the first output row of row i.
__global__ void __launch_bounds__(kThreads)
    density_final_kernel(const uint32_t *__restrict__ action4, const uint32_t *__restrict__ bsum, int64_t n,
                         uint32_t *__restrict__ prefix) {
    __shared__ uint32_t lds[kThreads];
    const int64_t r0 = (int64_t)blockIdx.x * kDensityScanRows + threadIdx.x * kScanPer;
    const uint32_t word = action4[(size_t)blockIdx.x * kThreads + threadIdx.x];
    uint32_t cnt[kScanPer], sum = 0u;
#pragma unroll
    for (int k = 0; k < kScanPer; ++k) {
        cnt[k] = rows_of((word >> (8 * k)) & 0xffu);
        sum += cnt[k];
    }
    uint32_t total;
    uint32_t at = bsum[blockIdx.x] + block_exclusive(sum, lds, total);
#pragma unroll
    for (int k = 0; k < kScanPer; ++k) {
        if (r0 + k < n) prefix[r0 + k] = at;
        at += cnt[k];
    }
}

// kinds of an output row in the run's table: entry = local source row | kind << 8
enum : uint32_t { kContinued = 0, kCloneNew = 1, kChild0 = 2, kChild1 = 3 };

__device__ __forceinline__ float run_element(const float *__restrict__ src, uint32_t w, int role, float shrink,
                                             const uint32_t *table, const float *offset, uint32_t j, uint32_t kk) {
    const uint32_t entry = table[j], r = entry & 0xffu, kind = entry >> 8;
    if (role == GSX_DENSITY_ZERO_NEW && kind != kContinued) return 0.0f;
    float v = src[r * w + kk];
    if (kind >= kChild0) {
        if (role == GSX_DENSITY_SCALES) v = v / shrink;
        if (role == GSX_DENSITY_POINTS) v = v + offset[3 * j + kk];
    }
    return v;
}

__global__ void __launch_bounds__(kDensityRows) density_apply_kernel(const DensityArgs k, int64_t n_out) {
    __shared__ uint32_t table[2 * kDensityRows];
    __shared__ float offset[2 * kDensityRows * 3];
    __shared__ uint32_t span[2];
    const uint32_t tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * kDensityRows, row = row0 + tid;
    const int64_t left = k.n - row0;
    const uint32_t rows = left < (int64_t)kDensityRows ? (uint32_t)left : (uint32_t)kDensityRows;
    const uint32_t action = tid < rows ? (uint32_t)k.action[row] : (uint32_t)kDensityPrune;
    const uint32_t cnt = rows_of(action), first = tid < rows ? k.prefix[row] : 0u;
    if (tid == 0) span[0] = first;
    if (tid == rows - 1u) span[1] = first + cnt;
    table[tid] = 0u;                    // (an entry a broken plan leaves out reads the block's first row, which exists)
    table[tid + kDensityRows] = 0u;
    __syncthreads();
    const uint32_t out0 = span[0], run = span[1] - out0;
    // (a plan is trusted only as far as it stays inside the arrays: at most 512 rows, all of them below n_out)
    if (run == 0u || run > 2u * kDensityRows || (int64_t)out0 + run > n_out) return;
    const uint32_t local = first - out0;
    if (cnt != 0u && local + cnt <= run) {
        const uint32_t kind0 = action == kDensitySplit ? kChild0 : kContinued;
        table[local] = tid | (kind0 << 8);
        if (cnt == 2u) table[local + 1u] = tid | ((action == kDensitySplit ? kChild1 : kCloneNew) << 8);
        if (k.source_row) {
            k.source_row[(int64_t)out0 + local] = kind0 == kContinued ? (int32_t)row : -(int32_t)(row + 1);
            if (cnt == 2u) k.source_row[(int64_t)out0 + local + 1] = -(int32_t)(row + 1);
        }
        if (action == kDensitySplit && k.noise) {
            const float *q = k.quats + 4 * row, *s = k.scales + 3 * row, *e = k.noise + 6 * row;
            const float nrm = sqrtf(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
            float w = 1.0f, x = 0.0f, y = 0.0f, z = 0.0f;
            if (nrm > 0.0f) {
                w = q[0] / nrm; x = q[1] / nrm; y = q[2] / nrm; z = q[3] / nrm;
            }
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
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const float d0 = s[0] * e[3 * c], d1 = s[1] * e[3 * c + 1], d2 = s[2] * e[3 * c + 2];
#pragma unroll
                for (int kk = 0; kk < 3; ++kk)
                    offset[3 * (local + c) + kk] = (R[kk][0] * d0 + R[kk][1] * d1) + R[kk][2] * d2;
            }
        }
    }
    __syncthreads();
    const float shrink = *k.shrink;

    for (int gi = 0; gi < k.n_groups; ++gi) {
        const DensityGroupArgs &G = k.group[gi];
        const uint32_t w = (uint32_t)G.width, count = run * w;
        const int role = G.role;
        const float *src = G.src + row0 * (int64_t)w;
        float *dst = G.dst + (int64_t)out0 * (int64_t)w;
        uint32_t lead = (4u - ((uint32_t)(reinterpret_cast<uintptr_t>(dst) >> 2) & 3u)) & 3u;
        lead = lead < count ? lead : count;
        const uint32_t nvec = (count - lead) / 4u;
        // a width of whole quads between 16-byte aligned runs (the coefficients and their moments: four fifths of a trained
        // scene's bytes): no quad straddles a row, so a quad is one 16-byte load of its source row, or zeros
        if ((w & 3u) == 0u && lead == 0u && (reinterpret_cast<uintptr_t>(src) & 15u) == 0u && role != GSX_DENSITY_POINTS &&
            role != GSX_DENSITY_SCALES) {
            const uint32_t wq = w >> 2;
            for (uint32_t q = tid; q < nvec; q += kDensityRows) {
                const uint32_t j = q / wq, entry = table[j], r = entry & 0xffu;
                float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (role != GSX_DENSITY_ZERO_NEW || (entry >> 8) == kContinued)
                    v = reinterpret_cast<const float4 *>(src)[r * wq + (q - j * wq)];
                reinterpret_cast<float4 *>(dst)[q] = v;
            }
            continue;
        }
        for (uint32_t e = tid; e < lead; e += kDensityRows) {
            const uint32_t j = e / w;
            dst[e] = run_element(src, w, role, shrink, table, offset, j, e - j * w);
        }
        for (uint32_t q = tid; q < nvec; q += kDensityRows) {
            const uint32_t e0 = lead + 4u * q;
            uint32_t j = e0 / w, kk = e0 - j * w;
            float x[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                x[i] = run_element(src, w, role, shrink, table, offset, j, kk);
                if (++kk == w) { kk = 0u; ++j; }
            }
            *reinterpret_cast<float4 *>(dst + e0) = make_float4(x[0], x[1], x[2], x[3]);
        }
        for (uint32_t e = lead + 4u * nvec + tid; e < count; e += kDensityRows) {
            const uint32_t j = e / w;
            dst[e] = run_element(src, w, role, shrink, table, offset, j, e - j * w);
        }
    }
}

}  // namespace

hipError_t launch_density_accumulate(const float *grad, int32_t width, int64_t n, float *grad_sum, uint32_t *seen, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    density_accumulate_kernel<<<(unsigned)((n + kThreads - 1) / kThreads), kThreads, 0, s>>>(grad, (uint32_t)width, n, grad_sum, seen);
    return hipGetLastError();
}

hipError_t launch_density_plan(const float *grad_sum, const uint32_t *seen, const float *scales, const float *opacity_logit,
                               int64_t n, const GsxDensityRules &rules, char *ws, const DensityCarve &c, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const uint32_t nb = c.scan_blocks;
    uint32_t *action4 = reinterpret_cast<uint32_t *>(ws + c.action);
    uint32_t *bsum = reinterpret_cast<uint32_t *>(ws + c.bsum), *bpruned = bsum + nb + 1, *bsplit = bpruned + nb;
    density_classify_kernel<<<nb, kThreads, 0, s>>>(grad_sum, seen, scales, opacity_logit, n, rules, action4, bsum, bpruned, bsplit);
    return launch_density_plan_finish(n, rules.split_shrink, ws, c, s);
}

// The plan behind its classify launch (this file's or gsx_density_screen.hip's): block sums scanned, header, every row's place.
hipError_t launch_density_plan_finish(int64_t n, float split_shrink, char *ws, const DensityCarve &c, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const uint32_t nb = c.scan_blocks;
    uint32_t *action4 = reinterpret_cast<uint32_t *>(ws + c.action), *prefix = reinterpret_cast<uint32_t *>(ws + c.prefix);
    uint32_t *bsum = reinterpret_cast<uint32_t *>(ws + c.bsum), *bpruned = bsum + nb + 1, *bsplit = bpruned + nb;
    density_blocks_kernel<<<1, kThreads, 0, s>>>(bsum, bpruned, bsplit, nb, n, split_shrink, ws);
    density_final_kernel<<<nb, kThreads, 0, s>>>(action4, bsum, n, prefix);
    return hipGetLastError();
}

hipError_t launch_density_apply(const DensityArgs &args, int64_t n_out, hipStream_t s) {
    if (args.n <= 0 || n_out <= 0) return hipSuccess;
    density_apply_kernel<<<(unsigned)((args.n + kDensityRows - 1) / kDensityRows), kDensityRows, 0, s>>>(args, n_out);
    return hipGetLastError();
}

}  // namespace gsx
