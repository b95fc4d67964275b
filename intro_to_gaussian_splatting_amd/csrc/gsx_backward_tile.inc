// The compositing backward's tile kernel, included six times by gsx_backward.hip (inside its anonymous namespace):
//   GSX_TILE_KERNEL = backward_tile_kernel,          GSX_TILE_GEOMETRY = false: gsx_render_backward's, the colour-only instance
//   GSX_TILE_KERNEL = backward_tile_geometry_kernel, GSX_TILE_GEOMETRY = true:  gsx_render_backward_geometry's
//   GSX_TILE_KERNEL = backward_tile_depth_kernel,    GSX_TILE_GEOMETRY = true, GSX_TILE_DEPTH = 1: gsx_render_backward_depth's
//   GSX_TILE_KERNEL = backward_tile_abs_kernel,      GSX_TILE_GEOMETRY = true, GSX_TILE_ABS = 1: gsx_render_backward_screen_abs'
//   GSX_TILE_KERNEL = backward_tile_std_kernel,      GSX_TILE_GEOMETRY = false, GSX_TILE_STD = 1: gsx_render_backward_std's, colour-only
//   GSX_TILE_KERNEL = backward_tile_std_geometry_kernel, GSX_TILE_GEOMETRY = true, GSX_TILE_STD = 1: gsx_render_backward_std's
// Plain kernels from one text rather than a template or a shared device function: the colour-only kernel keeps its
// name and compiles to the instructions it had before the geometry instance existed, and both keep theirs beside the
// depth instance, whose text sits in #if GSX_TILE_DEPTH blocks, and beside the abs instance, whose text sits in
// #if GSX_TILE_ABS blocks.
//
// One wave per window tile.  Its pixels are taken 256 at a time (a 16x16 tile: once), four per lane; the list is staged
// 64 records per batch.  For a tile of more than 256 pixels the later chunks add their sums to the slots the first one
// stored (same wave, program order: no atomics).
// GEO (gsx_render_backward_geometry): with u = dL/dalpha alpha = dL/dpower and d = mean - pixel, also the five moments
// S1 = sum u d0, S2 = sum u d1, S3 = sum u d0^2, S4 = sum u d0 d1, S5 = sum u d1^2 of every record over the tile's
// pixels, into the pair's two float4 of bt.geo_slots: (S1, S2, S3, S4), (S5, 0, 0, 0).  Same walk, same stop rule; the
// four colour sums take the same operations in the same order as in the colour-only instance, whose code GEO = false
// leaves as it was.
// DEPTH (gsx_render_backward_depth): the geometry instance with two more channels per pixel, expected depth D = sum T alpha z
// and coverage A = sum T alpha, accumulated as depth_tile_kernel accumulates them (one fmaf, one add).  With gD = dL/dD and
// gA = dL/dA of the pixel, dL/dalpha gains T (z gD + gA) - ((D_fin - D_k) gD + (A_fin - A_k) gA) / (1 - alpha), added to the
// frame's two terms as separate addends BEFORE u is formed -- so the opacity sum and the five moments carry depth's share
// with no further code, and with gD = gA = +0 every sum is the geometry instance's, bit for bit (x + (+0) = x, and every
// accumulator starts at +0, so no -0 survives in either instance) -- and a sixth sum per record, Sz = sum T alpha gD =
// dL/dz, into the second float4 of the pair's geometry slot: (S5, Sz, 0, 0).
// ABS (gsx_render_backward_screen_abs): the geometry instance with two more sums per record, of the ABSOLUTE value of each
// pixel's term of dL/dmean = -1/2 (Q + Q^T) sum u d: Tx = sum |fmaf(2 q00, u d0, (q01 + q10) (u d1))| and
// Ty = sum |fmaf(q01 + q10, u d0, (2 q11) (u d1))|, u d0 and u d1 the very products S1 and S2 add up, into the free words of
// the second float4: (S5, 0, Tx, Ty).  The factor 1/2 is left to backward_geometry_abs_sum_kernel.  Every other sum takes the
// geometry instance's operations in its order.
// STD (gsx_render_backward_std; GSX_TILE_STD = 1, text in #if GSX_TILE_STD blocks): backward_tile_std_kernel (colour-only)
// and backward_tile_std_geometry_kernel walk the packed GSX_SEM_STD_3DGS records -- a = (x, y, Q''00, Qs''), b = (Q''11,
// opacity, r, g), c.x = b, exponent in log2 units -- under that rule set.  Per (pixel, record): pw and alpha =
// fminf(0.99f, op exp2(pw)) by the forward's operations (std_exponent), the forward's three decisions (std_tests: skip when
// pw > 0, skip when alpha < 1/255, stop BEFORE accumulating when T - T alpha < 1e-4), C_k by the forward's fmafs and
// T <- T - T alpha: the composited pairs are the forward's.  F is the forward's pixel, T_fin background included, so the
// background's share of dL/dalpha = T (c . g) - (F - C_k) . g / (1 - alpha) needs no code (alpha <= 0.99: the division is
// safe).  u = dL/dalpha alpha where the clamp is inactive (op exp2(pw) < 0.99f) and 0 where it is active: a clamped pair
// adds to dL/dc only.  u = dL/d(natural exponent); the moments are formed from it and d = mean - pixel as in GEO.  Pixels
// beyond the frame's width or height (partial edge tiles) start dead and read nothing.
#if GSX_TILE_DEPTH
__global__ void __launch_bounds__(64) GSX_TILE_ATTR GSX_TILE_KERNEL(BackwardTiles bt, TileGrid grid, OutDesc out, DepthTiles dt) {
#else
__global__ void __launch_bounds__(64) GSX_TILE_ATTR GSX_TILE_KERNEL(BackwardTiles bt, TileGrid grid, OutDesc out) {
#endif
    constexpr bool GEO = GSX_TILE_GEOMETRY;
    __shared__ float4 sa[64], sb[64], sc[64];
    __shared__ uint32_t sslot[64];
    __shared__ float ssum[64 * 4];
#if GSX_TILE_DEPTH
    constexpr int kGeoSums = 6;
    __shared__ float sz[64];
#elif GSX_TILE_ABS
    constexpr int kGeoSums = 7;
#else
    constexpr int kGeoSums = 5;
#endif
    __shared__ float sgeo[GEO ? 64 * kGeoSums : 1];
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
#if GSX_TILE_DEPTH
        float Dr[kNpx], Ar[kNpx], DF[kNpx], AF[kNpx], gD[kNpx], gA[kNpx];
#endif
#pragma unroll
        for (int j = 0; j < kNpx; ++j) {
            const int64_t p = chunk + j * 64 + lane;
#if GSX_TILE_STD
            live[j] = p < npx && tx * T + (int)(p % T) < grid.width && ty * T + (int)(p / T) < grid.height;
#else
            live[j] = p < npx;
#endif
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
#if GSX_TILE_DEPTH
            Dr[j] = Ar[j] = DF[j] = AF[j] = gD[j] = gA[j] = 0.0f;
            if (live[j]) {
                const int64_t at2 = depth_index(out, tx * T + x, ty * T + y);
                DF[j] = dt.depth[at2]; AF[j] = dt.depth[at2 + 1];
                gD[j] = dt.grad_depth[at2]; gA[j] = dt.grad_depth[at2 + 1];
            }
#endif
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
#if GSX_TILE_DEPTH
                sz[lane] = dt.zrow[row];
#endif
                sslot[lane] = bt.prefix[rank] + (uint32_t)(tx - R.x0) * h + (uint32_t)(ty - R.y0);
            }
            __syncthreads();
            for (uint32_t k = 0; k < cnt; ++k) {
                bool any = false;
#pragma unroll
                for (int j = 0; j < kNpx; ++j) any |= live[j];
                float d0 = 0.0f, d1 = 0.0f, d2 = 0.0f, du = 0.0f;
                float m1 = 0.0f, m2 = 0.0f, m3 = 0.0f, m4 = 0.0f, m5 = 0.0f;
#if GSX_TILE_DEPTH
                float mz = 0.0f;
#endif
#if GSX_TILE_ABS
                float mx = 0.0f, my = 0.0f;
#endif
                if (__any(any)) {
                    const float4 A = sa[k], B = sb[k], Cc = sc[k];
#if GSX_TILE_DEPTH
                    const float zk = sz[k];
#endif
#if GSX_TILE_ABS
                    const float qxx = 2.0f * A.z, qxy = A.w + B.x, qyy = 2.0f * B.y;      // Q + Q^T
#endif
#pragma unroll
                    for (int j = 0; j < kNpx; ++j) {
                        if (!live[j]) continue;
#if GSX_TILE_STD
                        const float e0 = A.x - fx[j], e1 = A.y - fy[j];
                        const float pw = std_exponent(e0, e1, A.z, A.w, B.x);
                        const float raw = B.y * __builtin_amdgcn_exp2f(pw);
                        const float alpha = fminf(kStdAlphaMax, raw);
                        float ta;
                        bool use, stop;
                        std_tests(pw, alpha, kStdAlphaMin, Tr[j], ta, use, stop);
                        if (stop) {                     // the pixel stops before this record
                            live[j] = false;
                            continue;
                        }
                        if (!use) continue;             // skipped by one of the two skip rules
                        C0[j] = __builtin_fmaf(ta, B.z, C0[j]);
                        C1[j] = __builtin_fmaf(ta, B.w, C1[j]);
                        C2[j] = __builtin_fmaf(ta, Cc.x, C2[j]);
                        const float cg = (B.z * G0[j] + B.w * G1[j]) + Cc.x * G2[j];
                        const float rest = ((F0[j] - C0[j]) * G0[j] + (F1[j] - C1[j]) * G1[j]) + (F2[j] - C2[j]) * G2[j];
                        const float da = Tr[j] * cg - rest / (1.0f - alpha);
                        d0 = __builtin_fmaf(ta, G0[j], d0);
                        d1 = __builtin_fmaf(ta, G1[j], d1);
                        d2 = __builtin_fmaf(ta, G2[j], d2);
                        const float u = raw < kStdAlphaMax ? da * alpha : 0.0f;     // a clamped alpha is a constant
                        du += u;
                        if constexpr (GEO) {
                            const float u0 = u * e0, u1 = u * e1;
                            m1 += u0;
                            m2 += u1;
                            m3 = __builtin_fmaf(u0, e0, m3);
                            m4 = __builtin_fmaf(u0, e1, m4);
                            m5 = __builtin_fmaf(u1, e1, m5);
                        }
                        Tr[j] = Tr[j] - ta;
#else
                        const float alpha = alpha_ref_walk(A.x, A.y, A.z, A.w, B.x, B.y, B.z, fx[j], fy[j]);
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
#if GSX_TILE_DEPTH
                        Dr[j] = __builtin_fmaf(ta, zk, Dr[j]);
                        Ar[j] += ta;
                        const float zg = zk * gD[j] + gA[j];
                        const float restd = (DF[j] - Dr[j]) * gD[j] + (AF[j] - Ar[j]) * gA[j];
                        const float da = Tr[j] * (cg + zg) - (rest + restd) / (1.0f - alpha);
                        mz = __builtin_fmaf(ta, gD[j], mz);
#else
                        const float da = Tr[j] * cg - rest / (1.0f - alpha);
#endif
                        d0 = __builtin_fmaf(ta, G0[j], d0);
                        d1 = __builtin_fmaf(ta, G1[j], d1);
                        d2 = __builtin_fmaf(ta, G2[j], d2);
                        du = __builtin_fmaf(da, alpha, du);
                        if constexpr (GEO) {
                            // (alpha_ref_tail: where v_exp_f32 flushed alpha to zero the moments still get their terms)
                            const float ag = alpha_ref_tail(A.x, A.y, A.z, A.w, B.x, B.y, B.z, fx[j], fy[j], alpha);
                            const float u = da * ag, e0 = A.x - fx[j], e1 = A.y - fy[j];
                            const float u0 = u * e0, u1 = u * e1;
                            m1 += u0;
                            m2 += u1;
                            m3 = __builtin_fmaf(u0, e0, m3);
                            m4 = __builtin_fmaf(u0, e1, m4);
                            m5 = __builtin_fmaf(u1, e1, m5);
#if GSX_TILE_ABS
                            mx += fabsf(__builtin_fmaf(qxx, u0, qxy * u1));
                            my += fabsf(__builtin_fmaf(qxy, u0, qyy * u1));
#endif
                        }
                        Tr[j] = test;
#endif
                    }
                }
                const float v = wave_sum4(d0, d1, d2, du, lane);
                if ((lane & 15) == 0) ssum[k * 4 + (lane >> 4)] = v;
                if constexpr (GEO) {
                    const float w = wave_sum4(m1, m2, m3, m4, lane), w5 = wave_sum1(m5);
                    if ((lane & 15) == 0) sgeo[k * kGeoSums + (lane >> 4)] = w;
                    if (lane == 0) sgeo[k * kGeoSums + 4] = w5;
#if GSX_TILE_DEPTH
                    const float wz = wave_sum1(mz);
                    if (lane == 0) sgeo[k * kGeoSums + 5] = wz;
#endif
#if GSX_TILE_ABS
                    const float wxy = wave_sum2(mx, my, lane);
                    if ((lane & 31) == 0) sgeo[k * kGeoSums + 5 + (lane >> 5)] = wxy;      // Tx in lane 0, Ty in lane 32
#endif
                }
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
                if constexpr (GEO) {
                    const float *sg = sgeo + lane * kGeoSums;
                    float4 g0 = make_float4(sg[0], sg[1], sg[2], sg[3]);
#if GSX_TILE_DEPTH
                    float4 g1 = make_float4(sg[4], sg[5], 0.0f, 0.0f);
#elif GSX_TILE_ABS
                    float4 g1 = make_float4(sg[4], 0.0f, sg[5], sg[6]);
#else
                    float4 g1 = make_float4(sg[4], 0.0f, 0.0f, 0.0f);
#endif
                    float4 *gdst = bt.geo_slots + 2 * (size_t)sslot[lane];
                    if (chunk > 0) {
                        const float4 o0 = gdst[0], o1 = gdst[1];
                        g0 = make_float4(o0.x + g0.x, o0.y + g0.y, o0.z + g0.z, o0.w + g0.w);
                        g1.x += o1.x;
#if GSX_TILE_DEPTH
                        g1.y += o1.y;
#endif
#if GSX_TILE_ABS
                        g1.z += o1.z;
                        g1.w += o1.w;
#endif
                    }
                    gdst[0] = g0;
                    gdst[1] = g1;
                }
            }
            __syncthreads();
        }
    }
}

