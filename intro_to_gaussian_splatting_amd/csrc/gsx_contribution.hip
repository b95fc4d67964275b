// gsx_render_contribution: what every Gaussian adds to one frame -- per row the largest blend weight w = T alpha it reaches
// in any pixel (weight_max), the sum of its weights (weight_sum) and the number of pixels that composited it (pixels).
//
// The walk is the gradient entries' walk (gsx_backward.hip, gsx_backward_tile.inc), not the forward's: under GSX_SEM_REF_CPU
// alpha_ref_walk on every listed record with no 2^-26 skip and the pixel stopped before the record that fails kStopRefCpu, the
// raw stage-1 records (launch_project_raw); under GSX_SEM_STD_3DGS std_exponent and std_tests on the packed records of
// the frame's own projection, alpha = fminf(0.99, ..), pixels beyond the frame's width or height dead from the start.  For
// a composited (record, pixel) w is the very `ta` the backward instances form.
//
// Determinism, as in the backward: no float atomics.  (1) contribution_tile_kernel / contribution_tile_std_kernel: one wave
// per tile, four pixels per lane, 64 records staged per batch; per record the lane's four pixels are reduced in the lane,
// then over the wave by a fixed butterfly, and one 16-byte store leaves (max w, sum w, bits of the pixel count, 0) in the
// slot the (Gaussian, tile) pair had in the emission order.  A tile of more than 256 pixels goes in chunks, the later ones
// merging into the slot the first stored (fmaxf, +, +: same wave, program order).  (2) contribution_sum_kernel: one wave
// per depth rank reduces its contiguous slots, lane-strided and then by the butterfly; lane 0 owns the Gaussian's row and
// writes it, or merges into it (accumulate).
//
// weight_sum takes the colour-only backward instance's operations in its order -- d0 = fmaf(ta, G0, d0) with G0 = 1 is
// d0 + ta; wave_sum4's first component is x_l + x_(l+32), then the 16 .. 1 butterfly, which is the sum half of
// wave_sum_max below; the chunks add as o.x + v.x; the slots are summed as backward_sum_kernel sums them -- so it equals
// grad_colors[:, 0] of gsx_render_backward (gsx_render_backward_std) under dL/dframe = 1 bit for bit.
//
// Also here: the classify kernel of gsx_density_plan_contribution, which turns weight_max and views into a KEEP / PRUNE plan.
#include "gsx_density_device.h"

namespace gsx {
namespace {

constexpr int kNpx = 4;                   // pixels per lane of the tile kernels (a chunk = 256 pixels of the tile)

// Over the 64 lanes in a fixed order: the SUM of a, left in lane 0 (valid in lanes 0..31), and the MAX of b, left in lane 32
// (lanes 32..63).  The halves are exchanged with one shuffle, then each half reduces its value over its 32 lanes.  Six
// shuffles for both; the sum's order is that of the first component of gsx_backward.hip's wave_sum4.
__device__ __forceinline__ float wave_sum_max(float a, float b, int lane) {
    const bool up = (lane & 32) != 0;
    const float got = __shfl_xor(up ? a : b, 32);
    float v = up ? fmaxf(b, got) : a + got;
#pragma unroll
    for (int s = 16; s >= 1; s >>= 1) {
        const float o = __shfl_xor(v, s);
        v = up ? fmaxf(v, o) : v + o;
    }
    return v;
}

// What a wave leaves of one batch of records: the slot of every record's pair, merged when a later chunk of the tile's
// pixels finds what the first chunk stored.
__device__ __forceinline__ void store_batch(float4 *__restrict__ slots, const uint32_t *sslot, const float *smax,
                                            const float *ssum, const uint32_t *scnt, int lane, uint32_t cnt, bool merge) {
    if ((uint32_t)lane >= cnt) return;
    float4 *dst = slots + sslot[lane];
    float mx = smax[lane], sm = ssum[lane];
    uint32_t px = scnt[lane];
    if (merge) {
        const float4 o = *dst;
        mx = fmaxf(o.x, mx);
        sm = o.y + sm;
        px += __float_as_uint(o.z);
    }
    *dst = make_float4(mx, sm, __uint_as_float(px), 0.0f);
}

// One (pixel, record) pair under either rule set: whether the pixel composites the record; if so its weight ta = T alpha
// goes into the lane's sum and max and T is updated.  live: the pixel has not stopped (cleared here when it stops BEFORE
// this record).  kStd = false, GSX_SEM_REF_CPU: A = (x, y, Q00, Q01), B = (Q10, Q11, op, -) of the raw record, alpha_ref_walk and
// kStopRefCpu (a NaN stops too).  kStd = true, GSX_SEM_STD_3DGS: A = (x, y, Q''00, Qs''), B = (Q''11, opacity, ..) of the
// packed record, std_exponent and std_tests' two skips and stop.  The operations are the backward instances'.
template <bool kStd>
__device__ __forceinline__ bool composite_pair(const float4 &A, const float4 &B, float px, float py, bool &live, float &T,
                                               float &wsum, float &wmax) {
    bool used = false;
    if constexpr (kStd) {
        const float e0 = A.x - px, e1 = A.y - py;
        const float pw = std_exponent(e0, e1, A.z, A.w, B.x);
        const float alpha = fminf(kStdAlphaMax, B.y * __builtin_amdgcn_exp2f(pw));
        float ta;
        bool use, stop;
        std_tests(pw, alpha, kStdAlphaMin, T, ta, use, stop);
        if (stop) {                     // the pixel stops before this record
            live = false;
        } else if (use) {               // (else: skipped by one of the two skip rules)
            wsum += ta;
            wmax = fmaxf(wmax, ta);
            T = T - ta;
            used = true;
        }
    } else {
        const float alpha = alpha_ref_walk(A.x, A.y, A.z, A.w, B.x, B.y, B.z, px, py);
        const float ta = T * alpha;
        const float test = T - ta;
        if (!(test >= kStopRefCpu)) {   // the pixel stops before this record
            live = false;
        } else {
            wsum += ta;
            wmax = fmaxf(wmax, ta);
            T = test;
            used = true;
        }
    }
    return used;
}

// The tile walk of both rule sets: one wave per tile, four pixels per lane, 64 records staged per batch, a tile of more
// than 256 pixels in chunks.  kStd: pixels beyond the frame's width or height start dead (partial edge tiles).
template <bool kStd>
__device__ __forceinline__ void contribution_tile(const ContributionTiles &ct, const TileGrid &grid) {
    __shared__ float4 sa[64], sb[64];
    __shared__ uint32_t sslot[64], scnt[64];
    __shared__ float smax[64], ssum[64];
    const uint32_t t = blockIdx.x;
    const int lane = threadIdx.x;
    const uint32_t nwy = (uint32_t)grid.nwy();
    const int tx = grid.wx0 + (int)(t / nwy), ty = grid.wy0 + (int)(t % nwy);
    const uint2 rg = ct.ranges[t];
    const uint32_t first = rg.x, last = rg.y & ~kLongFlag;
    const int T = grid.tile;
    const int64_t npx = (int64_t)T * T;
    const float ox = (float)tx * (float)T, oy = (float)ty * (float)T;
    for (int64_t chunk = 0; chunk < npx; chunk += 64 * kNpx) {
        float fx[kNpx], fy[kNpx], Tr[kNpx];
        bool live[kNpx];
#pragma unroll
        for (int j = 0; j < kNpx; ++j) {
            const int64_t p = chunk + j * 64 + lane;
            live[j] = p < npx;
            if constexpr (kStd) live[j] = live[j] && tx * T + (int)(p % T) < grid.width && ty * T + (int)(p / T) < grid.height;
            const int x = live[j] ? (int)(p % T) : 0, y = live[j] ? (int)(p / T) : 0;
            fx[j] = ox + (float)x;
            fy[j] = oy + (float)y;
            Tr[j] = 1.0f;
        }
        for (uint32_t b = first; b < last; b += 64) {
            const uint32_t cnt = min(64u, last - b);
            if ((uint32_t)lane < cnt) {
                const uint32_t row = ct.vals[b + lane];
                const Record r = ct.raw[row];
                const uint32_t rank = ct.rank_of[row];
                const TileRect R = ct.rrect[rank];
                const uint32_t h = (uint32_t)(R.y1 - R.y0) + 1u;
                sa[lane] = r.a;
                sb[lane] = r.b;
                sslot[lane] = ct.prefix[rank] + (uint32_t)(tx - R.x0) * h + (uint32_t)(ty - R.y0);
            }
            __syncthreads();
            for (uint32_t k = 0; k < cnt; ++k) {
                bool any = false;
#pragma unroll
                for (int j = 0; j < kNpx; ++j) any |= live[j];
                float wsum = 0.0f, wmax = 0.0f;
                uint32_t wpx = 0u;
                if (__any(any)) {
                    const float4 A = sa[k], B = sb[k];
#pragma unroll
                    for (int j = 0; j < kNpx; ++j) {
                        bool used = false;
                        if (live[j]) used = composite_pair<kStd>(A, B, fx[j], fy[j], live[j], Tr[j], wsum, wmax);
                        wpx += (uint32_t)__popcll(__ballot(used));
                    }
                }
                // (wpx is the wave's own count, a scalar: a record no pixel of the chunk composited -- skipped everywhere, or
                // behind the last live pixel -- leaves the +0 / +0 the butterfly would have produced, without its shuffles)
                const float v = wpx != 0u ? wave_sum_max(wsum, wmax, lane) : 0.0f;
                if (lane == 0) {
                    ssum[k] = v;
                    scnt[k] = wpx;
                }
                if (lane == 32) smax[k] = v;
            }
            __syncthreads();
            store_batch(ct.slots, sslot, smax, ssum, scnt, lane, cnt, chunk > 0);
            __syncthreads();
        }
    }
}

// GSX_SEM_REF_CPU: depth_tile_kernel's walk with the pair slots of backward_tile_kernel.
__global__ void __launch_bounds__(64) contribution_tile_kernel(ContributionTiles ct, TileGrid grid) {
    contribution_tile<false>(ct, grid);
}

// GSX_SEM_STD_3DGS: backward_tile_std_kernel's walk on the packed records.
__global__ void __launch_bounds__(64) contribution_tile_std_kernel(ContributionTiles ct, TileGrid grid) {
    contribution_tile<true>(ct, grid);
}

// One wave per depth rank: its slots [prefix[r], prefix[r + 1]) reduced lane-strided (the sum as backward_sum_kernel's
// first component), then over the wave; lane 0, the one owner of row order[r], writes the row or merges into it.
__global__ void __launch_bounds__(256)
    contribution_sum_kernel(const float4 *__restrict__ slots, const uint32_t *__restrict__ prefix,
                            const uint32_t *__restrict__ order, uint32_t m, float *__restrict__ weight_max,
                            float *__restrict__ weight_sum, uint32_t *__restrict__ pixels, uint32_t *__restrict__ views,
                            int accumulate) {
    const uint32_t r = (blockIdx.x * 256u + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (r >= m) return;
    const uint32_t b = prefix[r], e = prefix[r + 1];
    float a0 = 0.0f, mx = 0.0f;
    uint32_t px = 0u;
    for (uint32_t i = b + (uint32_t)lane; i < e; i += 64u) {
        const float4 v = slots[i];
        mx = fmaxf(mx, v.x);
        a0 += v.y;
        px += __float_as_uint(v.z);
    }
    const float v = wave_sum_max(a0, mx, lane);
    const float vmax = __shfl(v, 32);
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) px += __shfl_xor(px, s);
    if (lane == 0) {
        const uint32_t row = order[r];
        if (accumulate) {
            weight_max[row] = fmaxf(weight_max[row], vmax);
            weight_sum[row] = weight_sum[row] + v;
            pixels[row] = pixels[row] + px;
            if (views) views[row] = views[row] + 1u;
        } else {
            weight_max[row] = vmax;
            weight_sum[row] = v;
            pixels[row] = px;
            if (views) views[row] = 1u;
        }
    }
}

// gsx_density_plan_contribution's classify step: KEEP or PRUNE alone.  PRUNE where weight_max[i] < threshold (a NaN fails the
// comparison and is kept; equal is kept) and, with `views`, where no view listed the row (views[i] == 0), whatever its
// weight.  It leaves what density_classify_kernel leaves (gsx_density_device.h: leave_block), so the scan of the block sums
// and the rows' places are gsx_density.hip's kernels and the workspace feeds the unchanged gsx_density_apply.  It stands
// here, not beside its siblings: the kernel sets of gsx_density.hip and gsx_density_screen.hip are pinned by their tests.
__global__ void __launch_bounds__(density::kThreads)
    density_classify_contribution_kernel(const float *__restrict__ weight_max, const uint32_t *__restrict__ views, float threshold,
                                         int64_t n, uint32_t *__restrict__ action4, uint32_t *__restrict__ bsum,
                                         uint32_t *__restrict__ bpruned, uint32_t *__restrict__ bsplit) {
    using namespace density;
    __shared__ uint32_t lds[kThreads];
    const int64_t r0 = (int64_t)blockIdx.x * kDensityScanRows + threadIdx.x * kScanPer;
    uint32_t word = 0u, out = 0u, tally = 0u;
#pragma unroll
    for (int k = 0; k < kScanPer; ++k) {
        uint32_t a = kDensityPrune;
        if (r0 + k < n) {
            a = (weight_max[r0 + k] < threshold || (views && views[r0 + k] == 0u)) ? kDensityPrune : kDensityKeep;
            out += rows_of(a);
            tally += a == kDensityPrune ? 1u : 0u;
        }
        word |= a << (8 * k);
    }
    leave_block(word, out, tally, lds, action4, bsum, bpruned, bsplit);
}

}  // namespace

hipError_t launch_contribution_tiles(const ContributionTiles &ct, const TileGrid &grid, bool std_rules, hipStream_t s) {
    if (grid.count() <= 0) return hipSuccess;
    if (std_rules)
        contribution_tile_std_kernel<<<(unsigned)grid.count(), 64, 0, s>>>(ct, grid);
    else
        contribution_tile_kernel<<<(unsigned)grid.count(), 64, 0, s>>>(ct, grid);
    return hipGetLastError();
}

hipError_t launch_contribution_sums(const float4 *slots, const uint32_t *prefix, const uint32_t *order, uint32_t m,
                                    float *weight_max, float *weight_sum, uint32_t *pixels, uint32_t *views, bool accumulate,
                                    hipStream_t s) {
    if (m == 0) return hipSuccess;
    contribution_sum_kernel<<<(unsigned)(((uint64_t)m + 3) / 4), 256, 0, s>>>(slots, prefix, order, m, weight_max, weight_sum,
                                                                              pixels, views, accumulate ? 1 : 0);
    return hipGetLastError();
}

hipError_t launch_density_plan_contribution(const float *weight_max, const uint32_t *views, float threshold, int64_t n, char *ws,
                                            const DensityCarve &c, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const uint32_t nb = c.scan_blocks;
    uint32_t *action4 = reinterpret_cast<uint32_t *>(ws + c.action);
    uint32_t *bsum = reinterpret_cast<uint32_t *>(ws + c.bsum), *bpruned = bsum + nb + 1, *bsplit = bpruned + nb;
    density_classify_contribution_kernel<<<nb, density::kThreads, 0, s>>>(weight_max, views, threshold, n, action4, bsum, bpruned,
                                                                          bsplit);
    return launch_density_plan_finish(n, 1.0f, ws, c, s);      // (no row is split: the shrink factor is never read)
}

}  // namespace gsx
