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
// The file has two halves, each one text with an instance per entry.  Per pair: the tile walk (gsx_backward_tile.inc, six
// instances).  Per Gaussian: three bodies -- colour_sums (2), geometry_sums, which sums a second slot array the same way,
// and chain_rank, which carries those sums through stage 1's derivative (geometry_chain) -- behind one thin kernel per
// variant.  What each entry adds to gsx_render_backward:
// gsx_render_backward_geometry: dL/dpoint, dL/dscale, dL/dquaternion -- the gradients the reference's graph gives once its
// weight stays a tensor.  (1') backward_tile_geometry_kernel also sums five moments of u = dL/dalpha alpha per record into
// the second slot array; (2') backward_geometry_sum_kernel and backward_geometry_chain_kernel.  The colour-only kernels and
// their slots are the same code and layout either way.
// gsx_render_backward_screen: two more per-Gaussian stores in the chain: dL/d(NDC mean), which the chain forms anyway on its
// way to dL/dpoint, and the radius project_raw_kernel left in the raw record's last word.
// gsx_render_backward_camera: backward_camera_chain_kernel, the chain's g_t, dT and gh contracted with the point into 24
// terms of dL/dworld2view and dL/dfull_proj per Gaussian, summed per block with the butterflies above and LDS, and over the
// blocks by camera_reduce_kernel in a fixed order.
// gsx_render_depth and gsx_render_backward_depth: expected depth D = sum T alpha z and coverage A = sum T alpha per pixel
// (depth_tile_kernel, the backward's walk on the raw records plus one float per row, the view-space depth), and their
// gradients fused into the one backward walk: backward_tile_depth_kernel adds depth's term to dL/dalpha before u is formed
// and sums dL/dz per record beside the five moments; backward_depth_sum_kernel and backward_depth_chain_kernel carry that
// sixth sum, which reaches dL/dpoint through world2view's third column.
// gsx_render_backward_screen_abs: backward_tile_abs_kernel also sums the ABSOLUTE value of every pixel's term of dL/dmean per
// record, and backward_geometry_abs_sum_kernel sums those two beside the five moments, with one more store per Gaussian; the
// chain kernel is the geometry entry's.
// gsx_render_backward_std (GSX_SEM_STD_3DGS, and GSX_FLAG_ANTIALIASED): the tile walk's two std instances and the std and
// anti-aliased variants of the colour sums and of the chain.
//
// alpha is evaluated in the reference's operation order for every record (alpha_ref_walk and kStopRefCpu, gsx_internal.h: the
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

// Sum of one value over the 64 lanes in a fixed order (the butterfly of wave_sum4's last steps), left in every lane.
__device__ __forceinline__ float wave_sum1(float v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s);
    return v;
}

// Sums of a and of b over the 64 lanes in a fixed order, a's left in lanes 0..31 and b's in lanes 32..63: the halves are
// exchanged as in wave_sum4 (one shuffle), then the remaining value is reduced over the 32 lanes.  6 shuffles for two sums.
__device__ __forceinline__ float wave_sum2(float a, float b, int lane) {
    const bool up = (lane & 32) != 0;
    float v = up ? b : a;
    v += __shfl_xor(up ? a : b, 32);
#pragma unroll
    for (int s = 16; s >= 1; s >>= 1) v += __shfl_xor(v, s);
    return v;
}

// backward_tile_kernel, backward_tile_geometry_kernel, backward_tile_depth_kernel and backward_tile_abs_kernel: one text,
// four instances (gsx_backward_tile.inc)
#define GSX_TILE_STD 0
#define GSX_TILE_KERNEL backward_tile_kernel
#define GSX_TILE_GEOMETRY false
#define GSX_TILE_DEPTH 0
#define GSX_TILE_ABS 0
#define GSX_TILE_ATTR
#include "gsx_backward_tile.inc"
#undef GSX_TILE_KERNEL
#undef GSX_TILE_GEOMETRY
#undef GSX_TILE_ATTR
#define GSX_TILE_KERNEL backward_tile_geometry_kernel
#define GSX_TILE_GEOMETRY true
#define GSX_TILE_ATTR __attribute__((amdgpu_waves_per_eu(4, 4)))
#include "gsx_backward_tile.inc"
#undef GSX_TILE_KERNEL
#undef GSX_TILE_DEPTH
#undef GSX_TILE_ATTR
// the depth instance: 24 more live floats than the geometry instance's 108 VGPRs, left to the compiler's own occupancy
#define GSX_TILE_KERNEL backward_tile_depth_kernel
#define GSX_TILE_DEPTH 1
#define GSX_TILE_ATTR
#include "gsx_backward_tile.inc"
#undef GSX_TILE_KERNEL
#undef GSX_TILE_DEPTH
#undef GSX_TILE_ABS
#undef GSX_TILE_ATTR
// the abs instance: the geometry instance with two more accumulators and three hoisted conic sums, held to its occupancy
#define GSX_TILE_KERNEL backward_tile_abs_kernel
#define GSX_TILE_DEPTH 0
#define GSX_TILE_ABS 1
#define GSX_TILE_ATTR __attribute__((amdgpu_waves_per_eu(4, 4)))
#include "gsx_backward_tile.inc"
#undef GSX_TILE_KERNEL
#undef GSX_TILE_GEOMETRY
#undef GSX_TILE_DEPTH
#undef GSX_TILE_ABS
#undef GSX_TILE_ATTR
#undef GSX_TILE_STD
// the two GSX_SEM_STD_3DGS instances (gsx_render_backward_std): colour-only, and geometry held to the geometry instance's
// occupancy
#define GSX_TILE_STD 1
#define GSX_TILE_DEPTH 0
#define GSX_TILE_ABS 0
#define GSX_TILE_KERNEL backward_tile_std_kernel
#define GSX_TILE_GEOMETRY false
#define GSX_TILE_ATTR
#include "gsx_backward_tile.inc"
#undef GSX_TILE_KERNEL
#undef GSX_TILE_GEOMETRY
#undef GSX_TILE_ATTR
#define GSX_TILE_KERNEL backward_tile_std_geometry_kernel
#define GSX_TILE_GEOMETRY true
#define GSX_TILE_ATTR __attribute__((amdgpu_waves_per_eu(4, 4)))
#include "gsx_backward_tile.inc"
#undef GSX_TILE_KERNEL
#undef GSX_TILE_GEOMETRY
#undef GSX_TILE_DEPTH
#undef GSX_TILE_ABS
#undef GSX_TILE_ATTR
#undef GSX_TILE_STD

// gsx_render_depth: (D, A) = (sum T alpha z, sum T alpha) of every pixel of every window tile, by the backward's walk --
// one wave per tile, four pixels per lane, 64 records staged per batch, a tile of more than 256 pixels in chunks,
// alpha_ref_walk on every listed record (no 2^-26 skip), the pixel stopped before the record that fails kStopRefCpu.  D takes
// one fmaf per record and A one add: backward_tile_depth_kernel accumulates both the same way, so its D_fin - D_k and
// A_fin - A_k are exact zeros behind a pixel's last record.
__global__ void __launch_bounds__(64)
    depth_tile_kernel(const Record *__restrict__ raw, const uint32_t *__restrict__ vals, const uint2 *__restrict__ ranges,
                      const float *__restrict__ zrow, TileGrid grid, OutDesc out, float *__restrict__ depth) {
    __shared__ float4 sa[64], sb[64];
    __shared__ float sz[64];
    const uint32_t t = blockIdx.x;
    const int lane = threadIdx.x;
    const uint32_t nwy = (uint32_t)grid.nwy();
    const int tx = grid.wx0 + (int)(t / nwy), ty = grid.wy0 + (int)(t % nwy);
    const uint2 rg = ranges[t];
    const uint32_t first = rg.x, last = rg.y & ~kLongFlag;
    const int T = grid.tile;
    const int64_t npx = (int64_t)T * T;
    const float ox = (float)tx * (float)T, oy = (float)ty * (float)T;
    for (int64_t chunk = 0; chunk < npx; chunk += 64 * kNpx) {
        float fx[kNpx], fy[kNpx], Tr[kNpx], D[kNpx], A[kNpx];
        int64_t at[kNpx];
        bool live[kNpx], mine[kNpx];
#pragma unroll
        for (int j = 0; j < kNpx; ++j) {
            const int64_t p = chunk + j * 64 + lane;
            live[j] = mine[j] = p < npx;
            const int x = live[j] ? (int)(p % T) : 0, y = live[j] ? (int)(p / T) : 0;
            fx[j] = ox + (float)x;
            fy[j] = oy + (float)y;
            Tr[j] = 1.0f;
            D[j] = A[j] = 0.0f;
            at[j] = depth_index(out, tx * T + x, ty * T + y);
        }
        for (uint32_t b = first; b < last; b += 64) {
            const uint32_t cnt = min(64u, last - b);
            if ((uint32_t)lane < cnt) {
                const uint32_t row = vals[b + lane];
                const Record r = raw[row];
                sa[lane] = r.a;
                sb[lane] = r.b;
                sz[lane] = zrow[row];
            }
            __syncthreads();
            bool any = false;
#pragma unroll
            for (int j = 0; j < kNpx; ++j) any |= live[j];
            if (__any(any)) {
                for (uint32_t k = 0; k < cnt; ++k) {
                    const float4 Ra = sa[k], Rb = sb[k];
                    const float zk = sz[k];
#pragma unroll
                    for (int j = 0; j < kNpx; ++j) {
                        if (!live[j]) continue;
                        const float alpha = alpha_ref_walk(Ra.x, Ra.y, Ra.z, Ra.w, Rb.x, Rb.y, Rb.z, fx[j], fy[j]);
                        const float ta = Tr[j] * alpha;
                        const float test = Tr[j] - ta;
                        if (!(test >= kStopRefCpu)) {
                            live[j] = false;
                            continue;
                        }
                        D[j] = __builtin_fmaf(ta, zk, D[j]);
                        A[j] += ta;
                        Tr[j] = test;
                    }
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int j = 0; j < kNpx; ++j)
            if (mine[j]) {
                depth[at[j]] = D[j];
                depth[at[j] + 1] = A[j];
            }
    }
}

// ---- The per-Gaussian half: one body per role (colour sums, geometry sums, chain), one thin kernel per variant.
// The colour sums.  One wave per depth rank: its slots [prefix[r], prefix[r + 1]) summed lane-strided in rising order, then
// over the wave by wave_sum4's fixed butterfly; lane 0 writes the Gaussian's row (order[r]): the three colour sums, and
// dlogit(row, U, b, e) -- the rule set's way from the fourth sum U = sum u to dL/dlogit, the one thing the variants differ in.
// The kernels keep their pointers as __restrict__ arguments of their own and hand them on: what the compiler makes of the
// bodies rests on it (by-value structs in their place cost the chain kernels their register allocation).
template <class Logit>
__device__ __forceinline__ void colour_sums(const float4 *__restrict__ slots, const uint32_t *__restrict__ prefix,
                                            const uint32_t *__restrict__ order, uint32_t m, float *__restrict__ grad_colors,
                                            float *__restrict__ grad_opacity_logit, Logit dlogit) {
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
        const float dl = dlogit(row, u, b, e);
        grad_colors[3 * (int64_t)row] = v;
        grad_colors[3 * (int64_t)row + 1] = g;
        grad_colors[3 * (int64_t)row + 2] = bl;
        grad_opacity_logit[row] = dl;
    }
}

// GSX_SEM_REF_CPU: the raw record's b = (Q10, Q11, op = sigmoid(s), s = sigmoid(logit)), the sigmoid applied twice.
__global__ void __launch_bounds__(256)
    backward_sum_kernel(const float4 *__restrict__ slots, const uint32_t *__restrict__ prefix, const uint32_t *__restrict__ order,
                        const Record *__restrict__ raw, uint32_t m, float *__restrict__ grad_colors,
                        float *__restrict__ grad_opacity_logit) {
    colour_sums(slots, prefix, order, m, grad_colors, grad_opacity_logit, [=](uint32_t row, float u, uint32_t, uint32_t) {
        const float4 B = raw[row].b;
        const float ds = u * (1.0f - B.z);
        return ds * (B.w * (1.0f - B.w));
    });
}

// gsx_render_backward_std: the packed GSX_SEM_STD_3DGS record, b = (Q''11, op, r, g) with op = sigmoid(logit) applied ONCE.
__global__ void __launch_bounds__(256)
    backward_std_sum_kernel(const float4 *__restrict__ slots, const uint32_t *__restrict__ prefix,
                            const uint32_t *__restrict__ order, const Record *__restrict__ rec, uint32_t m,
                            float *__restrict__ grad_colors, float *__restrict__ grad_opacity_logit) {
    colour_sums(slots, prefix, order, m, grad_colors, grad_opacity_logit,
                [=](uint32_t row, float u, uint32_t, uint32_t) { return u * (1.0f - rec[row].b.y); });
}

// GSX_FLAG_ANTIALIASED: the record holds op_eff = sigmoid(logit) * rho (std_aa_factor), and alpha = op_eff G, so U is
// dL/d ln op_eff: dL/dlogit = U (1 - sigmoid(logit)), the sigmoid formed from the opacity input by stage 1's own operations
// (std_sigmoid).  The chain after this kernel needs U for dL/drho: lane 0 leaves it in the free second word of the Gaussian's
// first geometry slot pair, which backward_geometry_sum_kernel -- launched BEFORE this kernel on that path -- has already
// rewritten as (S5, 0, 0, 0).  No extra pass, no atomics.  geo_slots null: the colour-only call.
__global__ void __launch_bounds__(256)
    backward_std_aa_sum_kernel(const float4 *__restrict__ slots, const uint32_t *__restrict__ prefix,
                               const uint32_t *__restrict__ order, const float *__restrict__ opacity_logit, uint32_t m,
                               float *__restrict__ grad_colors, float *__restrict__ grad_opacity_logit,
                               float4 *__restrict__ geo_slots) {
    colour_sums(slots, prefix, order, m, grad_colors, grad_opacity_logit, [=](uint32_t row, float u, uint32_t b, uint32_t e) {
        if (geo_slots && b != e) geo_slots[2 * (size_t)b + 1].y = u;
        return u * (1.0f - std_sigmoid(opacity_logit[row]));
    });
}

// ---- gsx_render_backward_geometry: from a Gaussian's moment sums to dL/dpoint, dL/dscale, dL/dquaternion.
// What stage 1 computes (gsx_project.hip: project), differentiated by hand in float32.  With d = mean - pixel,
// power = -1/2 d^T Q d and u = dL/dpower:
//     dL/dQ_ij = -1/2 sum u d_i d_j              dL/dmean = -1/2 (Q + Q^T) sum u d
// (1) Q = adj(cov2d) / max(det, 1e-3), det = c00 c11 - c01 c10: where det is floored only the adjugate carries gradient
// (2) cov2d = (T Sigma T^T)[:2,:2], T = J W: dL/dSigma = T^T G T, dL/dT = G T Sigma^T + G^T T Sigma, dL/dJ = dL/dT W^T;
//     J00 = fx / z, J02 = -fx cx / z^2, J11 = fy / z, J12 = -fy cy / z^2 with cx = clamp(tx / z, +-1.3 tan_fovx) z:
//     where the clamp is active d cx / d tx = 0 and d cx / d z = the clamp value
// (3) Sigma = M M^T, M = R diag(s): dL/dM = (dL/dSigma + dL/dSigma^T) M, dL/ds_j = sum_i dL/dM_ij R_ij, dL/dR_ij = dL/dM_ij s_j
// (4) R of the quaternion normalised twice: each normalisation b = a / |a| maps g to (g - b (b . g)) / |a|
// (5) pixel mean = ((h_xy / h_w) + 1)(dim - 1) / 2, h = [p, 1] @ full_proj
// (6) dL/dpoint = (5) through full_proj plus the view-space point's gradient of (2) through world2view
// The branch decisions of (1) and (2) are taken on float32 values computed by the forward's operations in the forward's
// order (ewa_covariance and finish_projection of gsx_project.hip, rows class kRowsMany); the rest of the forward values
// this needs are recomputed in whatever order is shortest: they enter the gradient as factors, not as decisions.
// kStd (gsx_render_backward_std): the same chain through GSX_SEM_STD_3DGS's stage 1 (gsx_project.hip: project_std), which
// differs in five places -- (4) the quaternion is normalised once; (2) cov00 += 0.3 and cov11 += 0.3, constants, and the one
// off-diagonal entry c01 serves for both (c10 = c01), so its gradient is the sum of the two; (1) Q = adj / det with no floor;
// (5) pixel mean = ((h_xy p_w + 1) dim - 1) / 2 with p_w = 1 / (h_w + 1e-7), so d pixel / d ndc = dim / 2 (cam.sx, cam.sy)
// and the focal lengths are dim / (2 tan(fov / 2)) (cam.fx, cam.fy).  The packed record holds Q'' = -1/2 log2(e) Q, not Q:
// the conic is formed here as project_std forms it, and so is the published radius ceil(3 sqrt(lambda_max)) (*rad).
// kAa (GSX_FLAG_ANTIALIASED, with kStd): alpha = sigmoid(logit) rho G with rho = sqrt(det0 / det1) of the covariance before
// and after the dilation (std_aa_factor: the forward's own float32 decision), so U = sum u = dL/d ln rho and step (1) gains
//     ln rho = 1/2 (ln det0 - ln det1):   g_ca += 1/2 U (cd0 / det0 - cd1 / det1),   g_cd += 1/2 U (ca0 / det0 - ca1 / det1),
//     off-diagonal total -U cb (1 / det0 - 1 / det1)
// before the c10 = c01 merge; where rho is clamped to its floor nothing is added.  The other instances' text is what it was.
struct GeoCamera {
    float V[16], F[16];            // world2view, full_proj (row vector times matrix)
    float fx, fy, limx, limy, sx, sy;   // focal lengths, 1.3 tan(fov / 2), (width - 1) / 2, (height - 1) / 2
};

// kCamera (gsx_render_backward_camera): also this Gaussian's 24 terms of dL/dworld2view and dL/dfull_proj into gc, the
// chain's own g_t, dT and gh contracted with the point instead of with the matrices (kCamTerms, below).  The other
// instance is the text it was: gc is never touched.
template <bool kCamera, bool kStd = false, bool kAa = false>
__device__ __forceinline__ void geometry_chain(const GeoCamera &cam, const float *__restrict__ p, const float *__restrict__ sc,
                                               const float *__restrict__ qin, const float4 QA, const float4 QB,
                                               float S1, float S2, float S3, float S4, float S5, float *__restrict__ gp,
                                               float *__restrict__ gs, float *__restrict__ gq, float *__restrict__ gn,
                                               float *__restrict__ gc, float *__restrict__ rad = nullptr, float U = 0.0f) {
    static_assert(kStd || !kAa, "the opacity compensation belongs to GSX_SEM_STD_3DGS");
    const float *V = cam.V, *F = cam.F;
    const float p0 = p[0], p1 = p[1], p2 = p[2];
    // ---- forward values
    // rotation, as covariance3d (gsx_project.hip) forms it
    const float n1 = fmaxf(sqrtf(((qin[0] * qin[0] + qin[1] * qin[1]) + qin[2] * qin[2]) + qin[3] * qin[3]), 1e-12f);
    const float a0 = qin[0] / n1, a1 = qin[1] / n1, a2 = qin[2] / n1, a3 = qin[3] / n1;
    float n2 = 1.0f, w = a0, x = a1, y = a2, z = a3;
    if constexpr (!kStd) {
        n2 = sqrtf(((a0 * a0 + a1 * a1) + a2 * a2) + a3 * a3);
        w = a0 / n2; x = a1 / n2; y = a2 / n2; z = a3 / n2;
    }
    float R[3][3], M[3][3], Sg[3][3];
    R[0][0] = 1.0f - 2.0f * (y * y + z * z);
    R[0][1] = 2.0f * (x * y - w * z);
    R[0][2] = 2.0f * (x * z + w * y);
    R[1][0] = 2.0f * (x * y + w * z);
    R[1][1] = 1.0f - 2.0f * (x * x + z * z);
    R[1][2] = 2.0f * (y * z - w * x);
    R[2][0] = 2.0f * (x * z - w * y);
    R[2][1] = 2.0f * (y * z + w * x);
    R[2][2] = 1.0f - 2.0f * (x * x + y * y);
    const float s3[3] = {sc[0], sc[1], sc[2]};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) M[i][j] = R[i][j] * s3[j];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) Sg[i][j] = (M[i][0] * M[j][0] + M[i][1] * M[j][1]) + M[i][2] * M[j][2];
    // view-space point and the clamp, as ewa_covariance forms them
    float t[3];
#pragma unroll
    for (int c = 0; c < 3; ++c)
        t[c] = __builtin_fmaf(p2, V[8 + c], __builtin_fmaf(p1, V[4 + c], p0 * V[c])) + V[12 + c];
    const float tz = t[2];
    const float rx = t[0] / tz, ry = t[1] / tz;
    const float kx = fminf(fmaxf(rx, -cam.limx), cam.limx), ky = fminf(fmaxf(ry, -cam.limy), cam.limy);
    const bool inx = rx >= -cam.limx && rx <= cam.limx, iny = ry >= -cam.limy && ry <= cam.limy;
    const float cx = kx * tz, cy = ky * tz;
    const float z2 = tz * tz;
    const float j00 = cam.fx / tz, j02 = -(cam.fx * cx) / z2, j11 = cam.fy / tz, j12 = -(cam.fy * cy) / z2;
    float T[2][3], B[2][3], C[2][3];       // T = J W, W[i][j] = V[j * 4 + i]; B = T Sigma; C = B W^T
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        T[0][j] = __builtin_fmaf(j02, V[j * 4 + 2], j00 * V[j * 4 + 0]);
        T[1][j] = __builtin_fmaf(j12, V[j * 4 + 2], j11 * V[j * 4 + 1]);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) B[i][j] = (T[i][0] * Sg[0][j] + T[i][1] * Sg[1][j]) + T[i][2] * Sg[2][j];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            C[i][j] = __builtin_fmaf(B[i][2], V[2 * 4 + j], __builtin_fmaf(B[i][1], V[1 * 4 + j], B[i][0] * V[0 * 4 + j]));
    float ca = C[0][0] * j00 + C[0][2] * j02, cb = C[0][1] * j11 + C[0][2] * j12;
    float cc = C[1][0] * j00 + C[1][2] * j02, cd = C[1][1] * j11 + C[1][2] * j12;
    const float ca0 = ca, cd0 = cd;         // (read by kAa only)
    if constexpr (kStd) {
        ca = ca + 0.3f;
        cd = cd + 0.3f;
        cc = cb;
    }
    const float det_raw = ca * cd - cb * cc;
    const float det = kStd ? det_raw : fmaxf(det_raw, 1e-3f);
    const bool floored = !kStd && det_raw < 1e-3f;
    // ---- compositing: dL/dQ and dL/dmean (Q as the record stores it)
    float q00 = QA.z, q01 = QA.w, q10 = QB.x, q11 = QB.y;
    if constexpr (kStd) {       // the conic and the radius as project_std forms them
        const float det_inv = 1.0f / det;
        q00 = cd * det_inv;
        q01 = -cb * det_inv;
        q10 = q01;
        q11 = ca * det_inv;
        const float mid = 0.5f * (ca + cd);
        const float root = sqrtf(fmaxf(0.1f, mid * mid - det));
        *rad = ceilf(3.0f * sqrtf(fmaxf(mid + root, mid - root)));
    }
    const float gq00 = -0.5f * S3, gq01 = -0.5f * S4, gq11 = -0.5f * S5;       // gq10 = gq01
    const float gmx = -0.5f * (2.0f * q00 * S1 + (q01 + q10) * S2);
    const float gmy = -0.5f * ((q01 + q10) * S1 + 2.0f * q11 * S2);
    // ---- (1)
    float g_ca = gq11 / det, g_cd = gq00 / det, g_cb = -gq01 / det, g_cc = -gq01 / det;
    if (!floored) {
        const float g_det = -(((gq00 * q00 + gq01 * q01) + gq01 * q10) + gq11 * q11) / det;
        g_ca += g_det * cd;
        g_cd += g_det * ca;
        g_cb -= g_det * cc;
        g_cc -= g_det * cb;
    }
    if constexpr (kAa) {
        const StdAaFactor f = std_aa_factor(ca0, cb, cd0, det);
        if (!f.clamped) {
            const float hu = 0.5f * U;
            g_ca += hu * (cd0 / f.det0 - cd / det);
            g_cd += hu * (ca0 / f.det0 - ca / det);
            g_cb += -(U * cb) * (1.0f / f.det0 - 1.0f / det);
        }
    }
    if constexpr (kStd) {       // c10 = c01: one entry carries both
        g_cb += g_cc;
        g_cc = 0.0f;
    }
    // ---- (2): G = [[g_ca, g_cb], [g_cc, g_cd]]
    float GT[2][3], GtT[2][3];             // G T and G^T T
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        GT[0][j] = g_ca * T[0][j] + g_cb * T[1][j];
        GT[1][j] = g_cc * T[0][j] + g_cd * T[1][j];
        GtT[0][j] = g_ca * T[0][j] + g_cc * T[1][j];
        GtT[1][j] = g_cb * T[0][j] + g_cd * T[1][j];
    }
    float dS[3][3], dT[2][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) dS[i][j] = T[0][i] * GT[0][j] + T[1][i] * GT[1][j];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            dT[i][j] = ((GT[i][0] * Sg[j][0] + GT[i][1] * Sg[j][1]) + GT[i][2] * Sg[j][2]) +
                       ((GtT[i][0] * Sg[0][j] + GtT[i][1] * Sg[1][j]) + GtT[i][2] * Sg[2][j]);
    // dL/dJ_ik = sum_j dT_ij W_kj, W_kj = V[j * 4 + k]
    const float gj00 = (dT[0][0] * V[0] + dT[0][1] * V[4]) + dT[0][2] * V[8];
    const float gj02 = (dT[0][0] * V[2] + dT[0][1] * V[6]) + dT[0][2] * V[10];
    const float gj11 = (dT[1][0] * V[1] + dT[1][1] * V[5]) + dT[1][2] * V[9];
    const float gj12 = (dT[1][0] * V[2] + dT[1][1] * V[6]) + dT[1][2] * V[10];
    const float z3 = z2 * tz;
    float g_t[3];
    const float g_cx = -gj02 * cam.fx / z2, g_cy = -gj12 * cam.fy / z2;
    g_t[2] = (-(gj00 * cam.fx) / z2 - (gj11 * cam.fy) / z2) + (gj02 * (2.0f * cam.fx * cx) / z3 + gj12 * (2.0f * cam.fy * cy) / z3);
    g_t[2] += g_cx * kx + g_cy * ky;
    const float g_rx = inx ? g_cx * tz : 0.0f, g_ry = iny ? g_cy * tz : 0.0f;
    g_t[0] = g_rx / tz;
    g_t[1] = g_ry / tz;
    g_t[2] -= (g_rx * t[0] + g_ry * t[1]) / z2;
    // ---- (3)
    float dM[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            dM[i][j] = ((dS[i][0] + dS[0][i]) * M[0][j] + (dS[i][1] + dS[1][i]) * M[1][j]) + (dS[i][2] + dS[2][i]) * M[2][j];
    float dR[3][3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        gs[j] = (dM[0][j] * R[0][j] + dM[1][j] * R[1][j]) + dM[2][j] * R[2][j];
#pragma unroll
        for (int i = 0; i < 3; ++i) dR[i][j] = dM[i][j] * s3[j];
    }
    // ---- (4)
    float gb[4];
    gb[0] = 2.0f * (((z * (dR[1][0] - dR[0][1])) + (y * (dR[0][2] - dR[2][0]))) + (x * (dR[2][1] - dR[1][2])));
    gb[1] = 2.0f * ((((y * (dR[0][1] + dR[1][0])) + (z * (dR[0][2] + dR[2][0]))) + (w * (dR[2][1] - dR[1][2]))) -
                    2.0f * x * (dR[1][1] + dR[2][2]));
    gb[2] = 2.0f * ((((x * (dR[0][1] + dR[1][0])) + (z * (dR[1][2] + dR[2][1]))) + (w * (dR[0][2] - dR[2][0]))) -
                    2.0f * y * (dR[0][0] + dR[2][2]));
    gb[3] = 2.0f * ((((x * (dR[0][2] + dR[2][0])) + (y * (dR[1][2] + dR[2][1]))) + (w * (dR[1][0] - dR[0][1]))) -
                    2.0f * z * (dR[0][0] + dR[1][1]));
    const float b4[4] = {w, x, y, z}, a4[4] = {a0, a1, a2, a3};
    const float bg = ((b4[0] * gb[0] + b4[1] * gb[1]) + b4[2] * gb[2]) + b4[3] * gb[3];
    float ga[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) ga[i] = (gb[i] - b4[i] * bg) / n2;
    const float ag = ((a4[0] * ga[0] + a4[1] * ga[1]) + a4[2] * ga[2]) + a4[3] * ga[3];
#pragma unroll
    for (int i = 0; i < 4; ++i) gq[i] = (ga[i] - a4[i] * ag) / n1;
    // ---- (5), (6)
    const float h0 = __builtin_fmaf(p2, F[8], __builtin_fmaf(p1, F[4], p0 * F[0])) + F[12];
    const float h1 = __builtin_fmaf(p2, F[9], __builtin_fmaf(p1, F[5], p0 * F[1])) + F[13];
    float h3 = __builtin_fmaf(p2, F[11], __builtin_fmaf(p1, F[7], p0 * F[3])) + F[15];
    if constexpr (kStd) h3 = h3 + 0.0000001f;
    const float gn0 = gmx * cam.sx, gn1 = gmy * cam.sy;     // dL/d(NDC mean): gsx_render_backward_screen's grad_means2d
    gn[0] = gn0;
    gn[1] = gn1;
    const float gh0 = gn0 / h3, gh1 = gn1 / h3;
    const float gh3 = -(gn0 * h0 + gn1 * h1) / (h3 * h3);
#pragma unroll
    for (int k = 0; k < 3; ++k)
        gp[k] = ((gh0 * F[k * 4] + gh1 * F[k * 4 + 1]) + gh3 * F[k * 4 + 3]) +
                ((g_t[0] * V[k * 4] + g_t[1] * V[k * 4 + 1]) + g_t[2] * V[k * 4 + 2]);
    if constexpr (kCamera) {
        // t_c = sum_k p_k V[k][c] + V[3][c]; T_ij = sum_k J_ik W_kj with W_kj = V[j][k]; h_c = sum_k p_k F[k][c] + F[3][c]
        const float J0[3] = {j00, 0.0f, j02}, J1[3] = {0.0f, j11, j12};
        const float gh[3] = {gh0, gh1, gh3}, pk[3] = {p0, p1, p2};
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                gc[k * 3 + c] = pk[k] * g_t[c] + (J0[c] * dT[0][k] + J1[c] * dT[1][k]);
                gc[12 + k * 3 + c] = pk[k] * gh[c];
            }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            gc[9 + c] = g_t[c];
            gc[21 + c] = gh[c];
        }
    }
}

// The geometry sums.  One wave per depth rank: the Gaussian's geometry slot pairs [prefix[r], prefix[r + 1]) summed as
// colour_sums sums the colour slots (lane-strided in rising order, then the fixed butterflies: wave_sum4 for the first four
// moments, wave_sum1 for S5).  The sums go back into the Gaussian's FIRST pair as (S1, S2, S3, S4), (S5, 0, 0, 0): only this
// wave reads the slots of rank r, and it has read them all by then.  A rank on no tile list is left alone.  Every kind forms
// the five moments in the same operations and the same order, so the chain behind any of them gives the same bits.
//   kDepth (gsx_render_backward_depth): the sixth sum Sz of the pairs' second .y, summed like S5; the pair becomes (S5, Sz, 0, 0).
//   kAbs (gsx_render_backward_screen_abs): the two absolute sums backward_tile_abs_kernel left in the pairs' second .z and .w,
//     Tx and Ty, summed like the moments and then by wave_sum2's fixed exchange and butterfly -- no atomics --, and a store
//     per Gaussian, grad_means2d_abs[row] = ((0.5f * Tx) * hx, (0.5f * Ty) * hy) with hx = |sx|, hy = |sy| the chain's half
//     extents.  The pair's .z and .w are read and then written as zeros; a rank on no tile list keeps the +0 the launch stored.
enum class GeoSums { kMoments, kDepth, kAbs };

template <GeoSums kKind>
__device__ __forceinline__ void geometry_sums(float4 *__restrict__ geo_slots, const uint32_t *__restrict__ prefix, uint32_t m,
                                              const uint32_t *__restrict__ order = nullptr, float hx = 0.0f, float hy = 0.0f,
                                              float *__restrict__ grad_means2d_abs = nullptr) {
    const uint32_t r = (blockIdx.x * 256u + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (r >= m) return;
    const uint32_t b = prefix[r], e = prefix[r + 1];
    if (b == e) return;
    float a1 = 0.0f, a2 = 0.0f, a3 = 0.0f, a4 = 0.0f, a5 = 0.0f, a6 = 0.0f, ax = 0.0f, ay = 0.0f;
    for (uint32_t i = b + (uint32_t)lane; i < e; i += 64u) {
        const float4 v = geo_slots[2 * (size_t)i], v5 = geo_slots[2 * (size_t)i + 1];
        a1 += v.x; a2 += v.y; a3 += v.z; a4 += v.w; a5 += v5.x;
        if constexpr (kKind == GeoSums::kDepth) a6 += v5.y;
        if constexpr (kKind == GeoSums::kAbs) { ax += v5.z; ay += v5.w; }
    }
    const float v = wave_sum4(a1, a2, a3, a4, lane);
    const float S5 = wave_sum1(a5);
    float Sz = 0.0f, Txy = 0.0f, Ty = 0.0f;
    if constexpr (kKind == GeoSums::kDepth) Sz = wave_sum1(a6);
    const float S2 = __shfl(v, 16), S3 = __shfl(v, 32), S4 = __shfl(v, 48);
    if constexpr (kKind == GeoSums::kAbs) {
        Txy = wave_sum2(ax, ay, lane);
        Ty = __shfl(Txy, 32);
    }
    if (lane == 0) {
        geo_slots[2 * (size_t)b] = make_float4(v, S2, S3, S4);
        geo_slots[2 * (size_t)b + 1] = make_float4(S5, Sz, 0.0f, 0.0f);
        if constexpr (kKind == GeoSums::kAbs) {
            const int64_t row = order[r];
            grad_means2d_abs[2 * row] = (0.5f * Txy) * hx;
            grad_means2d_abs[2 * row + 1] = (0.5f * Ty) * hy;
        }
    }
}

__global__ void __launch_bounds__(256)
    backward_geometry_sum_kernel(float4 *__restrict__ geo_slots, const uint32_t *__restrict__ prefix, uint32_t m) {
    geometry_sums<GeoSums::kMoments>(geo_slots, prefix, m);
}

__global__ void __launch_bounds__(256)
    backward_depth_sum_kernel(float4 *__restrict__ geo_slots, const uint32_t *__restrict__ prefix, uint32_t m) {
    geometry_sums<GeoSums::kDepth>(geo_slots, prefix, m);
}

__global__ void __launch_bounds__(256)
    backward_geometry_abs_sum_kernel(float4 *__restrict__ geo_slots, const uint32_t *__restrict__ prefix,
                                     const uint32_t *__restrict__ order, uint32_t m, float hx, float hy,
                                     float *__restrict__ grad_means2d_abs) {
    geometry_sums<GeoSums::kAbs>(geo_slots, prefix, m, order, hx, hy, grad_means2d_abs);
}

// The chain, for one depth rank r on a tile list, its first slot pair at b: the sums the geometry sums left there carried
// through geometry_chain, and the Gaussian's three rows (order[r]) written.  gsx_render_backward_screen (rows.grad_means2d not
// null) also gets the chain's dL/d(NDC mean) and the radius; the launch has zeroed both for the rows no kernel reaches.
//   kGeometry, kCamera (gc: the 24 camera terms, else not touched), kDepth: GSX_SEM_REF_CPU.  The conic comes from the raw
//     record, and rows.screen_radius (or null) gets the radius project_raw_kernel left in the record's last word.
//   kDepth (gsx_render_backward_depth): Sz world2view[k][2] added to dL/dpoint_k -- z = p . world2view[:3][2] + world2view[3][2]
//     -- as a separate addend and only where it is not zero: with dL/ddepth = 0 every row holds the screen entry's bits, a -0
//     included.
//   kStd, kStdAa (gsx_render_backward_std): the chain's kStd variant.  The packed record has no raw conic and no radius: the
//     chain forms both (no record is read), and rows.screen_radius is there whenever rows.grad_means2d is.  kStdAa
//     (GSX_FLAG_ANTIALIASED) is the chain's kAa variant; U = sum u is where backward_std_aa_sum_kernel left it, beside S5.
enum class Chain { kGeometry, kCamera, kDepth, kStd, kStdAa };

template <Chain kKind>
__device__ __forceinline__ void chain_rank(const float4 *__restrict__ geo_slots, const uint32_t *__restrict__ order,
                                           const Record *__restrict__ raw, const GeoCamera &cam, const GeometryRows &rows,
                                           uint32_t r, uint32_t b, float *__restrict__ gc) {
    constexpr bool kStd = kKind == Chain::kStd || kKind == Chain::kStdAa;
    const float4 S = geo_slots[2 * (size_t)b], S5 = geo_slots[2 * (size_t)b + 1];
    const int64_t row = order[r];
    float4 QA = make_float4(0.0f, 0.0f, 0.0f, 0.0f), QB = QA;
    float rad = 0.0f;
    if constexpr (!kStd) {
        const Record rec = raw[row];
        QA = rec.a;
        QB = rec.b;
        rad = rec.c.w;
    }
    float gp[3], gs[3], gq[4], gn[2];
    geometry_chain<kKind == Chain::kCamera, kStd, kKind == Chain::kStdAa>(
        cam, rows.means3d + 3 * row, rows.scales + 3 * row, rows.quats + 4 * row, QA, QB, S.x, S.y, S.z, S.w, S5.x, gp, gs, gq, gn,
        gc, &rad, kKind == Chain::kStdAa ? S5.y : 0.0f);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if constexpr (kKind == Chain::kDepth) {
            const float gz = S5.y * cam.V[k * 4 + 2];       // dL/dz dz/dp_k
            rows.grad_means3d[3 * row + k] = gz != 0.0f ? gp[k] + gz : gp[k];
        } else {
            rows.grad_means3d[3 * row + k] = gp[k];
        }
        rows.grad_scales[3 * row + k] = gs[k];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) rows.grad_quats[4 * row + k] = gq[k];
    if (rows.grad_means2d) {
        rows.grad_means2d[2 * row] = gn[0];
        rows.grad_means2d[2 * row + 1] = gn[1];
        if (kStd || rows.screen_radius) rows.screen_radius[row] = rad;
    }
}

// One thread per depth rank; a rank past m or on no tile list is left alone: its rows keep their zeros.
template <Chain kKind>
__device__ __forceinline__ void chain_ranks(const float4 *__restrict__ geo_slots, const uint32_t *__restrict__ prefix,
                                            const uint32_t *__restrict__ order, const Record *__restrict__ raw, uint32_t m,
                                            const GeoCamera &cam, const GeometryRows &rows) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= m) return;
    const uint32_t b = prefix[r];
    if (b == prefix[r + 1]) return;
    chain_rank<kKind>(geo_slots, order, raw, cam, rows, r, b, nullptr);
}

__global__ void __launch_bounds__(256)
    backward_geometry_chain_kernel(const float4 *__restrict__ geo_slots, const uint32_t *__restrict__ prefix,
                                   const uint32_t *__restrict__ order, const Record *__restrict__ raw, uint32_t m, GeoCamera cam,
                                   const float *__restrict__ means3d, const float *__restrict__ scales,
                                   const float *__restrict__ quats, float *__restrict__ grad_means3d,
                                   float *__restrict__ grad_scales, float *__restrict__ grad_quats,
                                   float *__restrict__ grad_means2d, float *__restrict__ screen_radius) {
    chain_ranks<Chain::kGeometry>(geo_slots, prefix, order, raw, m, cam,
                                  {means3d, scales, quats, grad_means3d, grad_scales, grad_quats, grad_means2d, screen_radius});
}

__global__ void __launch_bounds__(256)
    backward_depth_chain_kernel(const float4 *__restrict__ geo_slots, const uint32_t *__restrict__ prefix,
                                const uint32_t *__restrict__ order, const Record *__restrict__ raw, uint32_t m, GeoCamera cam,
                                const float *__restrict__ means3d, const float *__restrict__ scales,
                                const float *__restrict__ quats, float *__restrict__ grad_means3d,
                                float *__restrict__ grad_scales, float *__restrict__ grad_quats,
                                float *__restrict__ grad_means2d, float *__restrict__ screen_radius) {
    chain_ranks<Chain::kDepth>(geo_slots, prefix, order, raw, m, cam,
                               {means3d, scales, quats, grad_means3d, grad_scales, grad_quats, grad_means2d, screen_radius});
}

__global__ void __launch_bounds__(256)
    backward_std_chain_kernel(const float4 *__restrict__ geo_slots, const uint32_t *__restrict__ prefix,
                              const uint32_t *__restrict__ order, uint32_t m, GeoCamera cam, const float *__restrict__ means3d,
                              const float *__restrict__ scales, const float *__restrict__ quats, float *__restrict__ grad_means3d,
                              float *__restrict__ grad_scales, float *__restrict__ grad_quats, float *__restrict__ grad_means2d,
                              float *__restrict__ screen_radius) {
    chain_ranks<Chain::kStd>(geo_slots, prefix, order, nullptr, m, cam,
                             {means3d, scales, quats, grad_means3d, grad_scales, grad_quats, grad_means2d, screen_radius});
}

__global__ void __launch_bounds__(256)
    backward_std_aa_chain_kernel(const float4 *__restrict__ geo_slots, const uint32_t *__restrict__ prefix,
                                 const uint32_t *__restrict__ order, uint32_t m, GeoCamera cam, const float *__restrict__ means3d,
                                 const float *__restrict__ scales, const float *__restrict__ quats, float *__restrict__ grad_means3d,
                                 float *__restrict__ grad_scales, float *__restrict__ grad_quats, float *__restrict__ grad_means2d,
                                 float *__restrict__ screen_radius) {
    chain_ranks<Chain::kStdAa>(geo_slots, prefix, order, nullptr, m, cam,
                               {means3d, scales, quats, grad_means3d, grad_scales, grad_quats, grad_means2d, screen_radius});
}

// ---- gsx_render_backward_camera: dL/dworld2view and dL/dfull_proj, the 24 entries that are not exact zeros.
// kCamTerms values per Gaussian: [k * 3 + c] = dL/dV[k][c] (k < 4, c < 3; column 3 of V reaches nothing) and
// [12 + k * 3 + j] = dL/dF[k][c], c = (0, 1, 3)[j] (column 2 of F, the depth, reaches nothing).  The sum over Gaussians
// in a fixed order: within a wave the butterflies of wave_sum4, the block's four waves in wave order (LDS), one row of
// `partials` per block; camera_reduce_kernel then adds the rows in kCamStripes interleaved stripes, each in rising row
// order, and the stripes in stripe order.
constexpr int kCamTerms = 24, kCamStripes = 8;

// The chain with the camera terms: the geometry kernel's rows written with the same values, and no early return -- every
// thread of the block takes part in the reduction, a rank past m or on no tile list with 24 zeros.
__global__ void __launch_bounds__(256)
    backward_camera_chain_kernel(const float4 *__restrict__ geo_slots, const uint32_t *__restrict__ prefix,
                                 const uint32_t *__restrict__ order, const Record *__restrict__ raw, uint32_t m, GeoCamera cam,
                                 const float *__restrict__ means3d, const float *__restrict__ scales,
                                 const float *__restrict__ quats, float *__restrict__ grad_means3d,
                                 float *__restrict__ grad_scales, float *__restrict__ grad_quats,
                                 float *__restrict__ grad_means2d, float *__restrict__ screen_radius,
                                 float *__restrict__ partials) {
    __shared__ float lds[4][kCamTerms];
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float gc[kCamTerms];
#pragma unroll
    for (int i = 0; i < kCamTerms; ++i) gc[i] = 0.0f;
    uint32_t b = 0, e = 0;
    if (r < m) {
        b = prefix[r];
        e = prefix[r + 1];
    }
    if (b != e)
        chain_rank<Chain::kCamera>(geo_slots, order, raw, cam,
                                   {means3d, scales, quats, grad_means3d, grad_scales, grad_quats, grad_means2d, screen_radius}, r, b,
                                   gc);
#pragma unroll
    for (int g = 0; g < kCamTerms / 4; ++g) {
        const float v = wave_sum4(gc[4 * g], gc[4 * g + 1], gc[4 * g + 2], gc[4 * g + 3], lane);
        if ((lane & 15) == 0) lds[wave][4 * g + (lane >> 4)] = v;      // component v of the group sits in lane 16 v
    }
    __syncthreads();
    if (threadIdx.x < kCamTerms) {
        const int i = threadIdx.x;
        partials[(size_t)blockIdx.x * kCamTerms + i] = ((lds[0][i] + lds[1][i]) + lds[2][i]) + lds[3][i];
    }
}

// One workgroup of kCamStripes x 32 threads: thread (stripe, i) adds rows stripe, stripe + kCamStripes, .. of term i,
// thread i < 32 then adds the stripes and stores word i of both matrices (the eight structural zeros included).
__global__ void __launch_bounds__(kCamStripes * 32)
    camera_reduce_kernel(const float *__restrict__ partials, uint32_t rows, float *__restrict__ grad_world2view,
                         float *__restrict__ grad_full_proj) {
    __shared__ float lds[kCamStripes][kCamTerms];
    const int i = threadIdx.x & 31, stripe = threadIdx.x >> 5;
    if (i < kCamTerms) {
        float acc = 0.0f;
        for (uint32_t row = (uint32_t)stripe; row < rows; row += (uint32_t)kCamStripes) acc += partials[(size_t)row * kCamTerms + i];
        lds[stripe][i] = acc;
    }
    __syncthreads();
    if (threadIdx.x < 32) {
        // word t of the 32 outputs: V[k][c] for t < 16, F[k][c] behind; which of the 24 terms, or none
        const int t = threadIdx.x, k = (t & 15) >> 2, c = t & 3;
        const bool isV = t < 16;
        const int j = isV ? c : (c == 3 ? 2 : c);
        const bool zero = isV ? c == 3 : c == 2;
        float acc = 0.0f;
        if (!zero) {
            const int term = (isV ? 0 : 12) + k * 3 + j;
#pragma unroll
            for (int s = 0; s < kCamStripes; ++s) acc += lds[s][term];
        }
        (isV ? grad_world2view : grad_full_proj)[t & 15] = acc;
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
    if (bt.geo_slots)
        backward_tile_geometry_kernel<<<(unsigned)grid.count(), 64, 0, s>>>(bt, grid, out);
    else
        backward_tile_kernel<<<(unsigned)grid.count(), 64, 0, s>>>(bt, grid, out);
    return hipGetLastError();
}

hipError_t launch_backward_tiles_std(const BackwardTiles &bt, const TileGrid &grid, const OutDesc &out, hipStream_t s) {
    if (grid.count() <= 0) return hipSuccess;
    if (bt.geo_slots)
        backward_tile_std_geometry_kernel<<<(unsigned)grid.count(), 64, 0, s>>>(bt, grid, out);
    else
        backward_tile_std_kernel<<<(unsigned)grid.count(), 64, 0, s>>>(bt, grid, out);
    return hipGetLastError();
}

hipError_t launch_backward_tiles_abs(const BackwardTiles &bt, const TileGrid &grid, const OutDesc &out, hipStream_t s) {
    if (grid.count() <= 0) return hipSuccess;
    backward_tile_abs_kernel<<<(unsigned)grid.count(), 64, 0, s>>>(bt, grid, out);
    return hipGetLastError();
}

hipError_t launch_backward_tiles_depth(const BackwardTiles &bt, const DepthTiles &dt, const TileGrid &grid, const OutDesc &out,
                                       hipStream_t s) {
    if (grid.count() <= 0) return hipSuccess;
    backward_tile_depth_kernel<<<(unsigned)grid.count(), 64, 0, s>>>(bt, grid, out, dt);
    return hipGetLastError();
}

hipError_t launch_depth_tiles(const Record *raw, const uint32_t *vals, const uint2 *ranges, const float *zrow,
                              const TileGrid &grid, const OutDesc &out, float *depth, hipStream_t s) {
    if (grid.count() <= 0) return hipSuccess;
    depth_tile_kernel<<<(unsigned)grid.count(), 64, 0, s>>>(raw, vals, ranges, zrow, grid, out, depth);
    return hipGetLastError();
}

// Grids of 256 threads over m depth ranks: one wave per rank (the sums), one thread per rank (the chain).
static unsigned wave_blocks(uint32_t m) { return (unsigned)(((uint64_t)m + 3) / 4); }
static unsigned thread_blocks(uint32_t m) { return (unsigned)(((uint64_t)m + 255) / 256); }
// The eight rows as the chain kernels take them, one argument each
#define GSX_ROWS(rows) \
    (rows).means3d, (rows).scales, (rows).quats, (rows).grad_means3d, (rows).grad_scales, (rows).grad_quats, (rows).grad_means2d, \
        (rows).screen_radius

hipError_t launch_backward_sums(const RankSlots &rk, const Record *raw, float *grad_colors, float *grad_opacity_logit,
                                hipStream_t s) {
    if (rk.m == 0) return hipSuccess;
    backward_sum_kernel<<<wave_blocks(rk.m), 256, 0, s>>>(rk.slots, rk.prefix, rk.order, raw, rk.m, grad_colors, grad_opacity_logit);
    return hipGetLastError();
}

static GeoCamera geo_camera(const GsxCamera &camera) {
    GeoCamera cam;
    for (int i = 0; i < 16; ++i) {
        cam.V[i] = camera.world2view[i];
        cam.F[i] = camera.full_proj[i];
    }
    cam.fx = camera.fx;
    cam.fy = camera.fy;
    cam.limx = 1.3f * camera.tan_fovx;
    cam.limy = 1.3f * camera.tan_fovy;
    cam.sx = ((float)camera.width - 1.0f) * 0.5f;
    cam.sy = ((float)camera.height - 1.0f) * 0.5f;
    return cam;
}

// GSX_SEM_STD_3DGS: project_std's focal lengths and d pixel / d ndc
static GeoCamera geo_camera_std(const GsxCamera &camera) {
    GeoCamera cam = geo_camera(camera);
    cam.fx = (float)camera.width / (2.0f * camera.tan_fovx);
    cam.fy = (float)camera.height / (2.0f * camera.tan_fovy);
    cam.sx = (float)camera.width * 0.5f;
    cam.sy = (float)camera.height * 0.5f;
    return cam;
}

hipError_t launch_backward_geometry(const GsxCamera &camera, const RankSlots &rk, const Record *raw, const GeometryRows &rows,
                                    hipStream_t s, const CameraGrads *cg, float *grad_means2d_abs) {
    if (rk.m == 0) return hipSuccess;
    const GeoCamera cam = geo_camera(camera);
    if (grad_means2d_abs)
        backward_geometry_abs_sum_kernel<<<wave_blocks(rk.m), 256, 0, s>>>(rk.geo_slots, rk.prefix, rk.order, rk.m, fabsf(cam.sx),
                                                                           fabsf(cam.sy), grad_means2d_abs);
    else
        backward_geometry_sum_kernel<<<wave_blocks(rk.m), 256, 0, s>>>(rk.geo_slots, rk.prefix, rk.m);
    const unsigned blocks = thread_blocks(rk.m);
    if (cg) {
        backward_camera_chain_kernel<<<blocks, 256, 0, s>>>(rk.geo_slots, rk.prefix, rk.order, raw, rk.m, cam, GSX_ROWS(rows),
                                                            cg->partials);
        camera_reduce_kernel<<<1, kCamStripes * 32, 0, s>>>(cg->partials, blocks, cg->world2view, cg->full_proj);
        return hipGetLastError();
    }
    backward_geometry_chain_kernel<<<blocks, 256, 0, s>>>(rk.geo_slots, rk.prefix, rk.order, raw, rk.m, cam, GSX_ROWS(rows));
    return hipGetLastError();
}

hipError_t launch_backward_geometry_depth(const GsxCamera &camera, const RankSlots &rk, const Record *raw,
                                          const GeometryRows &rows, hipStream_t s) {
    if (rk.m == 0) return hipSuccess;
    backward_depth_sum_kernel<<<wave_blocks(rk.m), 256, 0, s>>>(rk.geo_slots, rk.prefix, rk.m);
    backward_depth_chain_kernel<<<thread_blocks(rk.m), 256, 0, s>>>(rk.geo_slots, rk.prefix, rk.order, raw, rk.m, geo_camera(camera),
                                                                    GSX_ROWS(rows));
    return hipGetLastError();
}

hipError_t launch_backward_sums_std(const RankSlots &rk, const Record *rec, float *grad_colors, float *grad_opacity_logit,
                                    hipStream_t s) {
    if (rk.m == 0) return hipSuccess;
    backward_std_sum_kernel<<<wave_blocks(rk.m), 256, 0, s>>>(rk.slots, rk.prefix, rk.order, rec, rk.m, grad_colors, grad_opacity_logit);
    return hipGetLastError();
}

hipError_t launch_backward_geometry_std(const GsxCamera &camera, const RankSlots &rk, const GeometryRows &rows, hipStream_t s) {
    if (rk.m == 0) return hipSuccess;
    backward_geometry_sum_kernel<<<wave_blocks(rk.m), 256, 0, s>>>(rk.geo_slots, rk.prefix, rk.m);
    backward_std_chain_kernel<<<thread_blocks(rk.m), 256, 0, s>>>(rk.geo_slots, rk.prefix, rk.order, rk.m, geo_camera_std(camera),
                                                                  GSX_ROWS(rows));
    return hipGetLastError();
}

hipError_t launch_backward_std_antialiased(const GsxCamera &camera, const RankSlots &rk, const GeometryRows &rows,
                                           const float *opacity_logit, float *grad_colors, float *grad_opacity_logit,
                                           hipStream_t s) {
    if (rk.m == 0) return hipSuccess;
    // the geometry sums first: they rewrite each Gaussian's first slot pair, whose free word then takes U from the colour sums
    if (rk.geo_slots) backward_geometry_sum_kernel<<<wave_blocks(rk.m), 256, 0, s>>>(rk.geo_slots, rk.prefix, rk.m);
    backward_std_aa_sum_kernel<<<wave_blocks(rk.m), 256, 0, s>>>(rk.slots, rk.prefix, rk.order, opacity_logit, rk.m, grad_colors,
                                                                 grad_opacity_logit, rk.geo_slots);
    if (rk.geo_slots)
        backward_std_aa_chain_kernel<<<thread_blocks(rk.m), 256, 0, s>>>(rk.geo_slots, rk.prefix, rk.order, rk.m,
                                                                         geo_camera_std(camera), GSX_ROWS(rows));
    return hipGetLastError();
}

}  // namespace gsx
