// gsx_knn3: for every point the exact distances to its three nearest other points, and the initial scale made of them.
//
// The reference states the rule (splat/gaussians.py:35-52, the mean of the three smallest neighbour distances) and leaves
// it switched off, because its n x n x 3 difference tensor does not fit.  The contract -- the float32 operation order of a
// squared distance, the two scale rules, +inf for a missing neighbour -- is include/gsx.h and is restated op for op in
// tests/knn_restatement.py; the library is built with -ffp-contract=off and correctly rounded sqrt and divide, and only the
// VALUES of the three smallest squared distances enter a result, so the kernel equals a brute force bit for bit whatever it
// prunes and in whatever order it meets the candidates.
//
// Gather: the points, in the caller's `order` (a Morton order makes the blocks compact), become float4 (x, y, z, row bits)
// entries; every kKnnRows = 256 consecutive entries get one box.
// Search: one workgroup per block, one query per thread, the best three squared distances in registers.  The own block is
// staged in LDS and scanned first, which gives every lane a third-best r3.  Then all boxes are tested, 256 at a time and one
// per thread, against the workgroup's largest r3 (refreshed before every 256 boxes); the survivors are listed in index
// order, and each listed block is staged (4 KiB, fetched into registers while the block before it is scanned) and scanned by
// the lanes whose own point-to-box bound is below their own r3.  All lanes read the same LDS address per candidate (a
// broadcast).  Tests skip on bound >= r3: an equal squared distance cannot change the three values, and a cloud of identical
// points stays linear.
#include <math.h>

#include "gsx_internal.h"

namespace gsx {
namespace {

constexpr int kThreads = kKnnRows, kWaves = kThreads / 64;
static_assert(kWaves == 4, "the workgroup reductions read four per-wave values");

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v = fminf(v, __shfl_xor(v, s));
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v = fmaxf(v, __shfl_xor(v, s));
    return v;
}

// The squared distance of the contract: every operation rounded on its own.
__device__ __forceinline__ float sq_dist(float px, float py, float pz, float x, float y, float z) {
    const float dx = x - px, dy = y - py, dz = z - pz;
    return (dx * dx + dy * dy) + dz * dz;
}

// A lower bound of sq_dist(p, x) over every x inside the box [lo, hi], EXACT in float32 as computed -- not only in the reals:
// per axis e = max(lo - p, 0, p - hi).  Rounding is monotone, so for every x >= lo, fl(x - p) >= fl(lo - p), and for every
// x <= hi, fl(p - x) >= fl(p - hi), with fl(x - p) = -fl(p - x): |fl(x - p)| >= e on every axis.  A rounded square and a
// rounded sum are monotone in non-negative operands, and the bound has the expression shape of sq_dist, so
// bound <= sq_dist(p, x) for every x in the box, as the kernel computes both.  The same holds box to box with
// e = max(lo_b - hi_a, 0, lo_a - hi_b): for every p <= hi_a, fl(lo_b - p) >= fl(lo_b - hi_a), so the box-to-box bound never
// exceeds the point-to-box bound of a point inside box a.
__device__ __forceinline__ float axis_gap(float lo_minus, float minus_hi) { return fmaxf(fmaxf(lo_minus, 0.0f), minus_hi); }
__device__ __forceinline__ float point_box(float px, float py, float pz, const float4 &lo, const float4 &hi) {
    const float ex = axis_gap(lo.x - px, px - hi.x), ey = axis_gap(lo.y - py, py - hi.y), ez = axis_gap(lo.z - pz, pz - hi.z);
    return (ex * ex + ey * ey) + ez * ez;
}
__device__ __forceinline__ float box_box(const float4 &alo, const float4 &ahi, const float4 &blo, const float4 &bhi) {
    const float ex = axis_gap(blo.x - ahi.x, alo.x - bhi.x), ey = axis_gap(blo.y - ahi.y, alo.y - bhi.y),
                ez = axis_gap(blo.z - ahi.z, alo.z - bhi.z);
    return (ex * ex + ey * ey) + ez * ez;
}

// Keeps the three smallest of (q0 <= q1 <= q2, q): values only, no branch.
__device__ __forceinline__ void keep3(float q, float &q0, float &q1, float &q2) {
    const float a = fmaxf(q0, q);
    q0 = fminf(q0, q);
    const float b = fmaxf(q1, a);
    q1 = fminf(q1, a);
    q2 = fminf(q2, b);
}

// Entries in `order` (an entry whose order[] is not a row falls back to its own index: the call stays inside its arrays)
// and the box of every block.  Entries behind n are not written; nothing reads them.
__global__ void __launch_bounds__(kThreads)
    knn_gather_kernel(const float *__restrict__ points, const int32_t *__restrict__ order, int64_t n, float4 *__restrict__ pts,
                      float4 *__restrict__ boxes) {
    __shared__ float red[kWaves][6];
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (e < n) {
        int64_t row = e;
        if (order) {
            const int64_t r = order[e];
            row = r >= 0 && r < n ? r : e;
        }
        const float x = points[3 * row], y = points[3 * row + 1], z = points[3 * row + 2];
        pts[e] = make_float4(x, y, z, __int_as_float((int32_t)row));
        lo[0] = hi[0] = x;
        lo[1] = hi[1] = y;
        lo[2] = hi[2] = z;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        lo[k] = wave_min(lo[k]);
        hi[k] = wave_max(hi[k]);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            red[wave][k] = lo[k];
            red[wave][3 + k] = hi[k];
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k)
            for (int w = 1; w < kWaves; ++w) {
                lo[k] = fminf(lo[k], red[w][k]);
                hi[k] = fmaxf(hi[k], red[w][3 + k]);
            }
        boxes[2 * (size_t)blockIdx.x] = make_float4(lo[0], lo[1], lo[2], 0.0f);
        boxes[2 * (size_t)blockIdx.x + 1] = make_float4(hi[0], hi[1], hi[2], 0.0f);
    }
}

__global__ void __launch_bounds__(kThreads)
    knn_search_kernel(const float4 *__restrict__ pts, const float4 *__restrict__ boxes, int64_t n, uint32_t nb, int32_t rule,
                      float *__restrict__ dist3, float *__restrict__ scale, unsigned long long *__restrict__ counter) {
    __shared__ float4 tile[kThreads];
    __shared__ uint32_t list[kThreads];
    __shared__ uint32_t wcnt[kWaves];
    __shared__ float wmax[kWaves];
    const uint32_t t = threadIdx.x, b = blockIdx.x, lane = t & 63u, wave = t >> 6;
    const int64_t base = (int64_t)b * kThreads;
    const uint32_t cnt = n - base < (int64_t)kThreads ? (uint32_t)(n - base) : (uint32_t)kThreads;
    const bool valid = t < cnt;
    float4 me = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (valid) me = pts[base + t];
    tile[t] = me;
    __syncthreads();

    // the own block: every other ENTRY (exclusion is by row, so a duplicate point counts, at distance 0)
    float q0 = INFINITY, q1 = INFINITY, q2 = INFINITY;
    uint32_t evaluated = 0u;
    if (valid) {
#pragma unroll 4
        for (uint32_t j = 0; j < cnt; ++j) {
            const float4 c = tile[j];
            const float q = sq_dist(me.x, me.y, me.z, c.x, c.y, c.z);
            keep3(j == t ? INFINITY : q, q0, q1, q2);
        }
        evaluated = cnt - 1u;
    }

    const float4 alo = boxes[2 * (size_t)b], ahi = boxes[2 * (size_t)b + 1];
    for (uint32_t b0 = 0; b0 < nb; b0 += kThreads) {
        // the workgroup's largest r3 as it is now (a lane without a query asks for nothing)
        const float mine = wave_max(valid ? q2 : -1.0f);
        if (lane == 0u) wmax[wave] = mine;
        const uint32_t ob = b0 + t;
        float bound = INFINITY;
        if (ob < nb && ob != b) bound = box_box(alo, ahi, boxes[2 * (size_t)ob], boxes[2 * (size_t)ob + 1]);
        __syncthreads();
        const float r3max = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
        const bool want = bound < r3max;
        const unsigned long long mask = __ballot(want);
        if (lane == 0u) wcnt[wave] = (uint32_t)__popcll(mask);
        __syncthreads();
        uint32_t at = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull)), total = 0u;
#pragma unroll
        for (uint32_t w = 0; w < (uint32_t)kWaves; ++w) {
            at += w < wave ? wcnt[w] : 0u;
            total += wcnt[w];
        }
        if (want) list[at] = ob;
        __syncthreads();
        if (total == 0u) continue;

        uint32_t next_ob = list[0];
        int64_t next_left = n - (int64_t)next_ob * kThreads;
        float4 next = make_float4(0.0f, 0.0f, 0.0f, 0.0f);     // (entries behind n: staged as zeros, scanned by nobody)
        if ((int64_t)t < next_left) next = pts[(int64_t)next_ob * kThreads + t];
        for (uint32_t i = 0; i < total; ++i) {
            const uint32_t cur = __builtin_amdgcn_readfirstlane(next_ob);
            const int64_t left = n - (int64_t)cur * kThreads;
            const uint32_t ocnt = left < (int64_t)kThreads ? (uint32_t)left : (uint32_t)kThreads;
            __syncthreads();            // everybody is done with the block staged before
            tile[t] = next;
            __syncthreads();
            if (i + 1u < total) {
                next_ob = list[i + 1u];
                next_left = n - (int64_t)next_ob * kThreads;
                if ((int64_t)t < next_left) next = pts[(int64_t)next_ob * kThreads + t];
            }
            const float4 blo = boxes[2 * (size_t)cur], bhi = boxes[2 * (size_t)cur + 1];
            if (valid && point_box(me.x, me.y, me.z, blo, bhi) < q2) {
#pragma unroll 4
                for (uint32_t j = 0; j < ocnt; ++j) {
                    const float4 c = tile[j];
                    keep3(sq_dist(me.x, me.y, me.z, c.x, c.y, c.z), q0, q1, q2);
                }
                evaluated += ocnt;
            }
        }
    }

    if (valid) {
        const int64_t row = (int64_t)__float_as_int(me.w);
        if (dist3) {
            dist3[3 * row] = sqrtf(q0);
            dist3[3 * row + 1] = sqrtf(q1);
            dist3[3 * row + 2] = sqrtf(q2);
        }
        if (scale) {
            if (rule == GSX_KNN_RULE_PUBLISHED)
                scale[row] = sqrtf(fmaxf(((q0 + q1) + q2) / 3.0f, 1e-7f));
            else
                scale[row] = fmaxf(((sqrtf(q0) + sqrtf(q1)) + sqrtf(q2)) / 3.0f, 1e-5f);
        }
    }
    if (counter) {
        uint32_t lo = evaluated & 0xffffu, hi = evaluated >> 16;      // 64 lanes of 16 bits each: no carry is lost
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {
            lo += __shfl_xor(lo, s);
            hi += __shfl_xor(hi, s);
        }
        // an integer sum: the same total in any order
        if (lane == 0u) atomicAdd(counter, ((unsigned long long)hi << 16) + (unsigned long long)lo);
    }
}

}  // namespace

hipError_t launch_knn3(const float *points, int64_t n, const int32_t *order, int32_t rule, float *dist3, float *scale, char *ws,
                       const KnnCarve &c, bool count, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    float4 *pts = reinterpret_cast<float4 *>(ws + c.pts), *boxes = reinterpret_cast<float4 *>(ws + c.boxes);
    knn_gather_kernel<<<c.blocks, kThreads, 0, s>>>(points, order, n, pts, boxes);
    knn_search_kernel<<<c.blocks, kThreads, 0, s>>>(pts, boxes, n, c.blocks, rule, dist3, scale,
                                                    count ? reinterpret_cast<unsigned long long *>(ws) : nullptr);
    return hipGetLastError();
}

}  // namespace gsx
