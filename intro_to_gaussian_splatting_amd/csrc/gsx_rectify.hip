// gsx_rectify_photo: one photograph resampled, under its COLMAP lens model, into the pinhole a rule set renders.
//
// BUILD EXTENSION -- the reference never reads a photograph.  The formula and its float32 operation order are the contract of
// include/gsx.h (gsx_rectify_photo) and are restated op for op in tests/rectify_restatement.py; the library is built with
// -ffp-contract=off, so every product, sum and quotient below rounds on its own (divide correctly rounded) and the outputs
// are reproducible from numpy.  One thread owns one output pixel (i, j): it walks its S x S sub-samples, b (along y) outer,
// a (along x) inner, sends each through the lens, decides validity, gathers four bilinear taps of three bytes and adds the
// sample's value to three running sums in that order.  No workspace, no atomics, no LDS, no cross-lane traffic: the same
// inputs give the same bits on every run.
//
// The block.  The output is (W', H', 3) with j = y contiguous, the photo (H, W, 3) with x contiguous: the store axis and
// the gather axis are crossed.  A wave laid along j alone stores 768 contiguous bytes but sends its 64 lanes to 64
// different photo rows, 64 cache lines per tap instruction, and the gather is what the kernel's time is.  A workgroup is
// kRectifyJ = 8 pixels along j by kRectifyI = 32 along i; a wave is 8 (j) x 8 (i): its stores are eight runs of 96 bytes,
// and the eight lanes that share a photo row sit within a few bytes of each other, so a tap instruction touches about 8
// rows, which the other waves of the block (the neighbouring i) find in the CU's cache.  Measured, 4000 x 3000 -> 1600 x
// 1200 at S = 3 on an MI355X (j x i): 64 x 4 0.189 ms, 32 x 8 0.171, 16 x 16 0.169, 8 x 32 0.089, 4 x 64 0.077,
// 2 x 128 0.085 ("Real captures": 4 x 64 was timed but the suite has not run on it; 8 x 32 is the shape
// every test ran with).  The photo is read byte by byte straight from global memory; an LDS-staged source tile was not
// tried.
#include "gsx_internal.h"

namespace gsx {
namespace {

__global__ void __launch_bounds__(kRectifyI * kRectifyJ) rectify_kernel(const RectifyArgs k) {
    const int j = blockIdx.x * kRectifyJ + (threadIdx.x % kRectifyJ);
    const int i = blockIdx.y * kRectifyI + (threadIdx.x / kRectifyJ);
    if (i >= k.out_w || j >= k.out_h) return;
    const int S = k.samples;
    const float Sf = (float)S;
    const float u_hi = (float)(k.src_w - 1), v_hi = (float)(k.src_h - 1);
    const float cxh = k.cxs - 0.5f, cyh = k.cys - 0.5f;
    const float k2x2 = 2.0f * k.k2, p1x2 = 2.0f * k.p1, p2x2 = 2.0f * k.p2, p1x6 = 6.0f * k.p1, p2x6 = 6.0f * k.p2;
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
    int count = 0;
    for (int b = 0; b < S; ++b) {
        const float y = (((float)j + (((float)b + 0.5f) / Sf - 0.5f)) - k.cy) / k.fy;
        const float yy = y * y;
        for (int a = 0; a < S; ++a) {
            const float x = (((float)i + (((float)a + 0.5f) / Sf - 0.5f)) - k.cx) / k.fx;
            const float xx = x * x, xy = x * y;
            const float r2 = xx + yy;
            const float rho = (k.k1 + k.k2 * r2) * r2;
            const float xd = ((x + x * rho) + p1x2 * xy) + k.p2 * (r2 + 2.0f * xx);
            const float yd = ((y + y * rho) + k.p1 * (r2 + 2.0f * yy)) + p2x2 * xy;
            const float g = 1.0f + rho;
            const float gp = k.k1 + k2x2 * r2;
            const float jxx = ((g + (2.0f * xx) * gp) + p1x2 * y) + p2x6 * x;
            const float jyy = ((g + (2.0f * yy) * gp) + p1x6 * y) + p2x2 * x;
            const float jxy = ((2.0f * xy) * gp + p1x2 * x) + p2x2 * y;
            const float det = jxx * jyy - jxy * jxy;
            const float u = k.fxs * xd + cxh;
            const float v = k.fys * yd + cyh;
            // (a NaN fails every comparison: nothing is gathered for it)
            if (!(u >= 0.0f && u <= u_hi && v >= 0.0f && v <= v_hi && det > 0.0f)) continue;
            const float fu = floorf(u), fv = floorf(v);
            const int x0 = (int)fu, y0 = (int)fv;
            const int x1 = min(x0 + 1, k.src_w - 1), y1 = min(y0 + 1, k.src_h - 1);   // u == W - 1: the tap's weight is 0
            const float tx = u - fu, ty = v - fv;
            const uint8_t *r0 = k.photo + (int64_t)y0 * k.row_stride, *r1 = k.photo + (int64_t)y1 * k.row_stride;
            const uint8_t *p00 = r0 + 3 * x0, *p01 = r0 + 3 * x1, *p10 = r1 + 3 * x0, *p11 = r1 + 3 * x1;
            float val[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float a00 = (float)p00[c], a01 = (float)p01[c], a10 = (float)p10[c], a11 = (float)p11[c];
                const float top = a00 + tx * (a01 - a00);
                const float bot = a10 + tx * (a11 - a10);
                val[c] = top + ty * (bot - top);
            }
            s0 = s0 + val[0];
            s1 = s1 + val[1];
            s2 = s2 + val[2];
            ++count;
        }
    }
    float *o = k.image + ((int64_t)i * k.out_h + j) * 3;
    if (count > 0) {
        const float den = 255.0f * (float)count;
        o[0] = s0 / den;
        o[1] = s1 / den;
        o[2] = s2 / den;
    } else {
        o[0] = 0.0f;
        o[1] = 0.0f;
        o[2] = 0.0f;
    }
    if (k.weight) k.weight[(int64_t)i * k.out_h + j] = (float)count / (float)(S * S);
}

}  // namespace

hipError_t launch_rectify(const RectifyArgs &args, hipStream_t s) {
    const dim3 grid((unsigned)((args.out_h + kRectifyJ - 1) / kRectifyJ), (unsigned)((args.out_w + kRectifyI - 1) / kRectifyI));
    rectify_kernel<<<grid, kRectifyI * kRectifyJ, 0, s>>>(args);
    return hipGetLastError();
}

}  // namespace gsx
