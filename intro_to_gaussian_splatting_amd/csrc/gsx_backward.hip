// Backward pass of the REF_CPU frame on gfx950: dL/dcolour and dL/dopacity-logit from dL/dframe.
//
// What the reference differentiates (paths relative to the reference repository): render_pixel
// (splat/gaussian_scene.py:146-171) builds every pixel from torch ops on the colours and on sigmoid(opacity) -- itself
// sigmoid(logit) from preprocess (:143) --, while the Gaussian weight w is a Python float (splat/utils.py:357-365,
// `.item()`): no gradient reaches the means, scales or quaternions.  Per pixel, with g = dL/dpixel, the list walked
// front to back under the reference's rule (alpha_k = w_k sigmoid(s_k), s_k = sigmoid(logit_k), stop BEFORE record k
// when T_k (1 - alpha_k) < 1e-6), C_fin the forward's pixel and C_k the running colour after record k:
//     dL/dc_k      = T_k alpha_k g
//     dL/dalpha_k  = T_k (c_k . g) - (C_fin - C_k) . g / (1 - alpha_k)
//     dL/ds_k      = dL/dalpha_k  w_k sigmoid(s_k) (1 - sigmoid(s_k)) = dL/dalpha_k  alpha_k (1 - sigmoid(s_k))
//     dL/dlogit_k  = dL/ds_k  s_k (1 - s_k)
// One front-to-back walk, the forward's own walk.  C_k is accumulated exactly like the forward accumulates it (one
// fmaf per channel), so C_fin - C_k is, to the rounding of those fmafs, the colour the records behind k added.  The
// division is safe for every composited record: T_k (1 - alpha_k) >= 1e-6 holds for each of them (a record with
// alpha >= 1 -- a "wild" footprint with a floored determinant, utils.py:383 -- stops the pixel).
//
// Determinism: no float atomics.  (1) backward_tile_kernel: one wave per tile walks its list; every record's four
// values (dL/dc rgb, sum of dL/dalpha alpha) are summed over the tile's pixels in a fixed order (in-lane over the
// lane's four pixels, then a fixed butterfly) and stored with one 16-B store into the slot the (Gaussian, tile) pair
// had in the EMISSION order of gsx_binning.hip: prefix[rank] + the tile's position in the Gaussian's rectangle, column
// by column.  (2) backward_sum_kernel: one wave per Gaussian sums its contiguous slots (lane-strided, then the same
// butterfly), applies the sigmoid chain and scatters to the Gaussian's row.  Same inputs, same bits.
//
// alpha is evaluated in the reference's operation order for every record (alpha_ref and kStopRefCpu, gsx_internal.h: the
// forward's own) and without the forward's 2^-26 skip: the gradient sees every record the reference sees.
#include "gsx_internal.h"

namespace gsx {
namespace {

constexpr int kScanThreads = 256, kScanPer = 4, kScanItems = kScanThreads * kScanPer;
constexpr int kNpx = 4;                   // pixels per lane of the tile kernel (a chunk = 256 pixels of the tile)

// Sum of (a, b, c, d) over the 64 lanes of the wave in a fixed order, left in lane 16 v of component v: halves are
// exchanged (32: (a,b) | (c,d); 16: one of the two), then the remaining value is reduced over the 16 lanes.  7 shuffles.
__device__ __forceinline__ float wave_sum4(float a, float b, float c, float d, int lane) {
    const bool up = (lane & 32) != 0;
    float k0 = up ? c : a, k1 = up ? d : b;
    k0 += __shfl_xor(up ? a : c, 32);
    k1 += __shfl_xor(up ? b : d, 32);
    const bool up2 = (lane & 16) != 0;
    float v = up2 ? k1 : k0;
    v += __shfl_xor(up2 ? k0 : k1, 16);
#pragma unroll
    for (int s = 8; s >= 1; s >>= 1) v += __shfl_xor(v, s);
    return v;
}

// Exclusive scan of one value per thread over the 256 threads of the workgroup; *total = the sum.
__device__ __forceinline__ uint32_t block_exclusive(uint32_t v, uint32_t *lds, uint32_t &total) {
    const int t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
#pragma unroll
    for (int s = 1; s < kScanThreads; s <<= 1) {
        const uint32_t add = t >= s ? lds[t - s] : 0u;
        __syncthreads();
        lds[t] += add;
        __syncthreads();
    }
    total = lds[kScanThreads - 1];
    const uint32_t incl = lds[t];
    __syncthreads();
    return incl - v;
}

// Per 1024 ranks: the sum of their tile counts (bsum[b]); rank_of[order[r]] = r.
__global__ void __launch_bounds__(kScanThreads)
    prefix_sums_kernel(const TileRect *__restrict__ rrect, const uint32_t *__restrict__ order, uint32_t m,
                       uint32_t *__restrict__ bsum, uint32_t *__restrict__ rank_of) {
    __shared__ uint32_t lds[kScanThreads];
    const uint32_t r0 = blockIdx.x * (uint32_t)kScanItems + threadIdx.x * kScanPer;
    uint32_t sum = 0;
#pragma unroll
    for (int k = 0; k < kScanPer; ++k) {
        const uint32_t r = r0 + k;
        if (r < m) {
            sum += tiles_of(rrect[r]);
            rank_of[order[r]] = r;
        }
    }
    uint32_t total;
    (void)block_exclusive(sum, lds, total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// One workgroup: exclusive scan of the nb block sums in place, bsum[nb] = their total (D).
__global__ void __launch_bounds__(kScanThreads) prefix_blocks_kernel(uint32_t *__restrict__ bsum, uint32_t nb) {
    __shared__ uint32_t lds[kScanThreads];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < nb; base += kScanThreads) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < nb ? bsum[i] : 0u;
        uint32_t total;
        const uint32_t ex = block_exclusive(v, lds, total);
        if (i < nb) bsum[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) bsum[nb] = carry;
}

// prefix[r] = emission slot of rank r's first pair; prefix[m] = D.
__global__ void __launch_bounds__(kScanThreads)
    prefix_final_kernel(const TileRect *__restrict__ rrect, uint32_t m, const uint32_t *__restrict__ bsum, uint32_t nb,
                        uint32_t *__restrict__ prefix) {
    __shared__ uint32_t lds[kScanThreads];
    const uint32_t r0 = blockIdx.x * (uint32_t)kScanItems + threadIdx.x * kScanPer;
    uint32_t cnt[kScanPer], sum = 0;
#pragma unroll
    for (int k = 0; k < kScanPer; ++k) {
        cnt[k] = r0 + k < m ? tiles_of(rrect[r0 + k]) : 0u;
        sum += cnt[k];
    }
    uint32_t total;
    uint32_t at = bsum[blockIdx.x] + block_exclusive(sum, lds, total);
#pragma unroll
    for (int k = 0; k < kScanPer; ++k) {
        if (r0 + k < m) prefix[r0 + k] = at;
        at += cnt[k];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) prefix[m] = bsum[nb];
}

// One wave per window tile.  Its pixels are taken 256 at a time (a 16x16 tile: once), four per lane; the list is staged
// 64 records per batch.  For a tile of more than 256 pixels the later chunks add their sums to the slots the first one
// stored (same wave, program order: no atomics).
__global__ void __launch_bounds__(64) backward_tile_kernel(BackwardTiles bt, TileGrid grid, OutDesc out) {
    __shared__ float4 sa[64], sb[64], sc[64];
    __shared__ uint32_t sslot[64];
    __shared__ float ssum[64 * 4];
    const uint32_t t = blockIdx.x;
    const int lane = threadIdx.x;
    const uint32_t nwy = (uint32_t)grid.nwy();
    const int tx = grid.wx0 + (int)(t / nwy), ty = grid.wy0 + (int)(t % nwy);
    const uint2 rg = bt.ranges[t];
    const uint32_t first = rg.x, last = rg.y & ~kLongFlag;
    const int T = grid.tile;
    const int64_t npx = (int64_t)T * T;
    const float ox = (float)tx * (float)T, oy = (float)ty * (float)T;
    for (int64_t chunk = 0; chunk < npx; chunk += 64 * kNpx) {
        float fx[kNpx], fy[kNpx], Tr[kNpx], C0[kNpx], C1[kNpx], C2[kNpx], F0[kNpx], F1[kNpx], F2[kNpx], G0[kNpx], G1[kNpx],
            G2[kNpx];
        bool live[kNpx];
#pragma unroll
        for (int j = 0; j < kNpx; ++j) {
            const int64_t p = chunk + j * 64 + lane;
            live[j] = p < npx;
            const int x = live[j] ? (int)(p % T) : 0, y = live[j] ? (int)(p / T) : 0;
            fx[j] = ox + (float)x;
            fy[j] = oy + (float)y;
            Tr[j] = 1.0f;
            C0[j] = C1[j] = C2[j] = 0.0f;
            F0[j] = F1[j] = F2[j] = G0[j] = G1[j] = G2[j] = 0.0f;
            if (live[j]) {
                const int64_t at = (int64_t)(tx * T + x - out.x0) * out.stride_x + (int64_t)(ty * T + y - out.y0) * out.stride_y;
                F0[j] = bt.image[at]; F1[j] = bt.image[at + 1]; F2[j] = bt.image[at + 2];
                G0[j] = bt.grad_image[at]; G1[j] = bt.grad_image[at + 1]; G2[j] = bt.grad_image[at + 2];
            }
        }
        for (uint32_t b = first; b < last; b += 64) {
            const uint32_t cnt = min(64u, last - b);
            if ((uint32_t)lane < cnt) {
                const uint32_t row = bt.vals[b + lane];
                const Record r = bt.raw[row];
                const uint32_t rank = bt.rank_of[row];
                const TileRect R = bt.rrect[rank];
                const uint32_t h = (uint32_t)(R.y1 - R.y0) + 1u;
                sa[lane] = r.a;
                sb[lane] = r.b;
                sc[lane] = r.c;
                sslot[lane] = bt.prefix[rank] + (uint32_t)(tx - R.x0) * h + (uint32_t)(ty - R.y0);
            }
            __syncthreads();
            for (uint32_t k = 0; k < cnt; ++k) {
                bool any = false;
#pragma unroll
                for (int j = 0; j < kNpx; ++j) any |= live[j];
                float d0 = 0.0f, d1 = 0.0f, d2 = 0.0f, du = 0.0f;
                if (__any(any)) {
                    const float4 A = sa[k], B = sb[k], Cc = sc[k];
#pragma unroll
                    for (int j = 0; j < kNpx; ++j) {
                        if (!live[j]) continue;
                        const float alpha = alpha_ref(A.x, A.y, A.z, A.w, B.x, B.y, B.z, fx[j], fy[j]);
                        const float ta = Tr[j] * alpha;
                        const float test = Tr[j] - ta;
                        if (!(test >= kStopRefCpu)) {   // the pixel stops before this record (the forward's rule; NaN stops too)
                            live[j] = false;
                            continue;
                        }
                        C0[j] = __builtin_fmaf(ta, Cc.x, C0[j]);
                        C1[j] = __builtin_fmaf(ta, Cc.y, C1[j]);
                        C2[j] = __builtin_fmaf(ta, Cc.z, C2[j]);
                        const float cg = (Cc.x * G0[j] + Cc.y * G1[j]) + Cc.z * G2[j];
                        const float rest = ((F0[j] - C0[j]) * G0[j] + (F1[j] - C1[j]) * G1[j]) + (F2[j] - C2[j]) * G2[j];
                        const float da = Tr[j] * cg - rest / (1.0f - alpha);
                        d0 = __builtin_fmaf(ta, G0[j], d0);
                        d1 = __builtin_fmaf(ta, G1[j], d1);
                        d2 = __builtin_fmaf(ta, G2[j], d2);
                        du = __builtin_fmaf(da, alpha, du);
                        Tr[j] = test;
                    }
                }
                const float v = wave_sum4(d0, d1, d2, du, lane);
                if ((lane & 15) == 0) ssum[k * 4 + (lane >> 4)] = v;
            }
            __syncthreads();
            if ((uint32_t)lane < cnt) {
                float4 v = make_float4(ssum[lane * 4], ssum[lane * 4 + 1], ssum[lane * 4 + 2], ssum[lane * 4 + 3]);
                float4 *dst = bt.slots + sslot[lane];
                if (chunk > 0) {
                    const float4 o = *dst;
                    v = make_float4(o.x + v.x, o.y + v.y, o.z + v.z, o.w + v.w);
                }
                *dst = v;
            }
            __syncthreads();
        }
    }
}

// One wave per depth rank: its slots [prefix[r], prefix[r + 1]) summed lane-strided, then over the wave; lane 0 applies
// the sigmoid chain and writes the Gaussian's row.
__global__ void __launch_bounds__(256)
    backward_sum_kernel(const float4 *__restrict__ slots, const uint32_t *__restrict__ prefix, const uint32_t *__restrict__ order,
                        const Record *__restrict__ raw, uint32_t m, float *__restrict__ grad_colors,
                        float *__restrict__ grad_opacity_logit) {
    const uint32_t r = (blockIdx.x * 256u + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (r >= m) return;
    const uint32_t b = prefix[r], e = prefix[r + 1];
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
    for (uint32_t i = b + (uint32_t)lane; i < e; i += 64u) {
        const float4 v = slots[i];
        a0 += v.x; a1 += v.y; a2 += v.z; a3 += v.w;
    }
    const float v = wave_sum4(a0, a1, a2, a3, lane);
    const float g = __shfl(v, 16), bl = __shfl(v, 32), u = __shfl(v, 48);
    if (lane == 0) {
        const uint32_t row = order[r];
        const float4 B = raw[row].b;        // (Q10, Q11, op = sigmoid(s), s = sigmoid(logit))
        const float ds = u * (1.0f - B.z);
        grad_colors[3 * (int64_t)row] = v;
        grad_colors[3 * (int64_t)row + 1] = g;
        grad_colors[3 * (int64_t)row + 2] = bl;
        grad_opacity_logit[row] = ds * (B.w * (1.0f - B.w));
    }
}

}  // namespace

hipError_t launch_backward_prefix(const TileRect *rrect, const uint32_t *order, uint32_t m, uint32_t *prefix,
                                  uint32_t *rank_of, uint32_t *bsum, hipStream_t s) {
    if (m == 0) return hipSuccess;
    const uint32_t nb = (m + kScanItems - 1) / kScanItems;
    prefix_sums_kernel<<<nb, kScanThreads, 0, s>>>(rrect, order, m, bsum, rank_of);
    prefix_blocks_kernel<<<1, kScanThreads, 0, s>>>(bsum, nb);
    prefix_final_kernel<<<nb, kScanThreads, 0, s>>>(rrect, m, bsum, nb, prefix);
    return hipGetLastError();
}

hipError_t launch_backward_tiles(const BackwardTiles &bt, const TileGrid &grid, const OutDesc &out, hipStream_t s) {
    if (grid.count() <= 0) return hipSuccess;
    backward_tile_kernel<<<(unsigned)grid.count(), 64, 0, s>>>(bt, grid, out);
    return hipGetLastError();
}

hipError_t launch_backward_sums(const float4 *slots, const uint32_t *prefix, const uint32_t *order, const Record *raw,
                                uint32_t m, float *grad_colors, float *grad_opacity_logit, hipStream_t s) {
    if (m == 0) return hipSuccess;
    backward_sum_kernel<<<(unsigned)(((uint64_t)m + 3) / 4), 256, 0, s>>>(slots, prefix, order, raw, m, grad_colors,
                                                                          grad_opacity_logit);
    return hipGetLastError();
}

}  // namespace gsx
