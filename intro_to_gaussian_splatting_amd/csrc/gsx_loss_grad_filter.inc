// The opening of the gradient kernel of both photometric losses, included once by each file, first thing between the braces of
//   loss_grad_kernel         gsx_loss.hip
//   wloss_grad_kernel<EXPO>  gsx_loss_weighted.hip
// No macro selects anything: the passage is the same in both.  Expected in scope: the arguments map_mu, map_p, map_q,
// map_stride, R, C, taps and tiles_c; gsx_loss_device.h.  It leaves to the kernel's own text: lds (kGradLds floats, free to
// reuse: the passage ends on a barrier), planes, hp, r0, c0, cf0, tr, tc and
//   F[k][ch][m]   the zero-padded 11 x 11 filter of map k (Dmu, Dp, Dq as the maps kernel stored them), channel ch, at this
//                 thread's output pixel m = (tr + (NT / T) m, tc) of the tile
// Each of the three maps in turn is staged with its halo, all three channels (zero outside the region, which is what makes
// the zero-padded filter its own adjoint; the maps' rows are always on stage_tile's 16-byte path), filtered along the row
// into LDS and along the column into registers.
// Text and not a __device__ __forceinline__ function, as gsx_loss_maps.inc: with this passage a function,
// loss_grad_kernel went from 81 to 82 VGPRs, one over its budget, and wloss_grad_kernel<false> from 82 to 74 -- other
// kernels, to be measured as such.  As text both compile to the instructions they had (docs/lab_notes/loss_shared_text.md).
    __shared__ __attribute__((aligned(16))) float lds[kGradLds];
    float *planes = lds, *hp = lds + 3 * kPlane;
    const uint32_t by = blockIdx.x / tiles_c, bx = blockIdx.x % tiles_c;
    const int64_t r0 = (int64_t)by * T, c0 = (int64_t)bx * T, cf0 = 3 * c0;
    const int tr = threadIdx.x / T, tc = threadIdx.x % T;
    float F[3][3][PX];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        stage_tile(k == 0 ? map_mu : (k == 1 ? map_p : map_q), map_stride, R, C, r0, cf0, planes, true);
        __syncthreads();
        for (int idx = threadIdx.x; idx < 3 * S * T; idx += NT) {
            const int ch = idx / (S * T), rem = idx % (S * T), i = rem / T, c = rem % T;
            float a = 0.0f;
#pragma unroll
            for (int t = 0; t < kTaps; ++t) a = fmaf(taps.g[t], planes[ch * kPlane + i * S + c + t], a);
            hp[idx] = a;
        }
        __syncthreads();
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
#pragma unroll
            for (int m = 0; m < PX; ++m) {
                const int r = tr + (NT / T) * m;
                float a = 0.0f;
#pragma unroll
                for (int t = 0; t < kTaps; ++t) a = fmaf(taps.g[t], hp[ch * S * T + (r + t) * T + tc], a);
                F[k][ch][m] = a;
            }
        __syncthreads();     // the next map overwrites planes and hp
    }
