// The body of the maps kernel of both photometric losses, included once by each file, between the braces of
//   loss_maps_kernel<GRAD>         gsx_loss.hip,          GSX_LOSS_WEIGHTED = 0
//   wloss_maps_kernel<GRAD, EXPO>  gsx_loss_weighted.hip, GSX_LOSS_WEIGHTED = 1
// The kernel's head stays with its file: name, template parameters, __launch_bounds__(NT) and arguments.  Expected in scope:
// the arguments image, image_stride, target, target_stride, R, C, taps, map_mu, map_p, map_q, map_stride, tiles_c, vec_x,
// vec_y of both; w and float2 *partials of the plain kernel; weight, weight_stride, exposure, float *sums, EXPO, Exposure,
// load_exposure, expose and kSums of the weighted one; gsx_loss_device.h.  Text in #if GSX_LOSS_WEIGHTED blocks is one
// kernel's alone; the three expressions in which the weight of output pixel m takes the place of the plain w = -lambda / n
// go through two macros, defined and #undef-ed here:
//   GSX_LOSS_SUM(m, v)   pixel m's term of a workgroup sum: v, or mw[m] v
//   GSX_LOSS_MAP(m)      the factor of pixel m's three map values: w, or mw[m] (1 / W is not known yet: the maps leave unscaled)
// Text and not a __device__ __forceinline__ function: the compiler allocates these large-LDS kernels differently when
// the passages reach it through a call.  With the SSIM passage as a function template over a weight policy,
// loss_maps_kernel<true> went from 100 to 80 VGPRs and wloss_maps_kernel<false, *> from 71 to 90 (its budget is 71); with
// the row store a function as well, loss_maps_kernel<true> took 159 VGPRs and 3 waves per SIMD, wloss_maps_kernel<true, *>
// 170 and 2.  As text every instance compiles to the instructions it had as a kernel written out in its own file
// (docs/lab_notes/loss_shared_text.md), which is what keeps the plain entry and the both-NULL route of the weighted one
// bit-compatible.
//
// One workgroup per 32 x 32 tile.  Both images' tile + 5-pixel halo go through LDS (stage_tile: loaded as the contiguous
// 3 (32 + 10) floats of a row, split into channel planes, zero outside the region).  Weighted: the staged x then becomes
// x' in place (a staged pixel inside the region: three reads, three writes by one thread; the zero padding stays zero, not
// E_i3), and the weight of an output pixel is one 4-byte read into a register.  Per channel the five quantities x, y, xx,
// xy, yy are filtered along the row into LDS and along the column into registers (explicit fmaf chains); then m, |x - y|
// and -- with a gradient -- Dmu, Dp, Dq times GSX_LOSS_MAP, which wait in registers until the last channel.  The sums leave
// through block_sum, one record per workgroup: (sum m, sum |x - y|), or (sum mw, sum mw m, sum mw |x' - y|).
    __shared__ __attribute__((aligned(16))) float lds[kMapsLds];
    float *px = lds, *py = lds + 3 * kPlane, *hp = lds + 6 * kPlane;
    const uint32_t by = blockIdx.x / tiles_c, bx = blockIdx.x % tiles_c;
    const int64_t r0 = (int64_t)by * T, c0 = (int64_t)bx * T, cf0 = 3 * c0;
    stage_tile(image, image_stride, R, C, r0, cf0, px, vec_x);
    stage_tile(target, target_stride, R, C, r0, cf0, py, vec_y);
    __syncthreads();
#if GSX_LOSS_WEIGHTED
    if (EXPO) {
        const Exposure E = load_exposure(exposure);
        for (int idx = threadIdx.x; idx < kPlane; idx += NT) {
            const int64_t rr = r0 - H + idx / S, cc = c0 - H + idx % S;
            if (rr >= 0 && rr < R && cc >= 0 && cc < C) {
                float xp[3];
                expose(E, px[idx], px[kPlane + idx], px[2 * kPlane + idx], xp);
                px[idx] = xp[0];
                px[kPlane + idx] = xp[1];
                px[2 * kPlane + idx] = xp[2];
            }
        }
        __syncthreads();
    }
#endif
    const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
    const int tr = threadIdx.x / T, tc = threadIdx.x % T;
#if GSX_LOSS_WEIGHTED
#define GSX_LOSS_SUM(m, v) mw[m] * (v)
#define GSX_LOSS_MAP(m) mw[m]
    float mw[PX];
    float sum_w = 0.0f, sum_m = 0.0f, sum_d = 0.0f;
#pragma unroll
    for (int m = 0; m < PX; ++m) {
        const int64_t row = r0 + tr + (NT / T) * m, col = c0 + tc;
        mw[m] = 0.0f;
        if (row < R && col < C) mw[m] = weight ? weight[row * weight_stride + col] : 1.0f;
        sum_w += mw[m];
    }
#else
#define GSX_LOSS_SUM(m, v) (v)
#define GSX_LOSS_MAP(m) w
    float sum_m = 0.0f, sum_d = 0.0f;
#endif
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
                sum_m += GSX_LOSS_SUM(m, mval);
                sum_d += GSX_LOSS_SUM(m, fabsf(x - y));
            }
            if (GRAD) {
                const float dmu = 2.0f * mu2 * (A2 - A1) / B12 - 2.0f * mu1 * A12 * (B2 - B1) / (B12 * B12);
                const float dp = -A12 / (B12 * B2);
                const float dq = 2.0f * A1 / B12;
                o[0][ch][m] = inside ? GSX_LOSS_MAP(m) * dmu : 0.0f;
                o[1][ch][m] = inside ? GSX_LOSS_MAP(m) * dp : 0.0f;
                o[2][ch][m] = inside ? GSX_LOSS_MAP(m) * dq : 0.0f;
            }
        }
        __syncthreads();     // the next channel overwrites hp
    }
#undef GSX_LOSS_SUM
#undef GSX_LOSS_MAP
    float *red = hp;
#if GSX_LOSS_WEIGHTED
    const float tot_w = block_sum(sum_w, red), tot_m = block_sum(sum_m, red), tot_d = block_sum(sum_d, red);
    if (threadIdx.x == 0) {
        float *dst = sums + (size_t)blockIdx.x * kSums;
        dst[0] = tot_w;
        dst[1] = tot_m;
        dst[2] = tot_d;
    }
#else
    const float tot_m = block_sum(sum_m, red), tot_d = block_sum(sum_d, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = make_float2(tot_m, tot_d);
#endif
    if (!GRAD) return;
    // the three maps leave as whole interleaved rows: obuf[map][r][3 c + ch] over the staging area, which nobody reads any
    // more; the maps' row stride is a multiple of 4 floats, so a quad inside the row is one 16-byte store, the tail goes
    // element by element
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
