// Internal declarations shared by the translation units of libgsx.so (not part of the ABI).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "gsx.h"
#include "gsx_plan.h"

namespace gsx {

// Measurement knobs (A/B runs of a kernel variant on the GPU box: tools/, bench.py --test-lib) exist only in
// libgsx_test.so, which is this same source built with -DGSX_TEST_HOOKS; in the shipping library knob() is its
// default and no environment variable is read anywhere.
inline int knob(const char *name, int dflt) {
#ifdef GSX_TEST_HOOKS
    const char *e = getenv(name);
    return e && *e ? atoi(e) : dflt;
#else
    (void)name;
    return dflt;
#endif
}

constexpr uint32_t kCulledKey = 0xFFFFFFFFu;  // depth key of a Gaussian behind the z >= 0.2 plane
constexpr uint32_t kEmptyKey = 0xFFFFFFFEu;   // visible, but it reaches no tile of the window; keys >= this are
                                              // dropped by the first pass of the depth sort

// Stage-1 -> stage-2 record, 48 B, three 16-B loads, indexed by the Gaussian's index (original
// index on the whole-path entry, row index on the stage-2 entry).  With Q'' = Q * (-1/2 log2 e):
//   GSX_SEM_REF_CPU (square completed in y, M = -Q'': r11 = sqrt(M11), h = M01 / r11, D1 = M00 - h^2):
//     a = (x_pix, y_pix, D1, h)   b = (r11, log2(opacity factor), r, g)   c = (b, depth, 0, -)
//     or, when that factorisation does not exist, the monomial form below with c.z = 1
//     or, for an ILL-CONDITIONED footprint (pack_record in gsx_project.hip), the same completed square with c = (b,
//     opacity factor, 2, -) and the raw float32 conic (Q00, Q01, Q10, Q11) in the Gaussian's slot of the per-Gaussian
//     float4 side array (the workspace's `bbox`): the compositing kernels execute the reference's own operation order
//     on such a record wherever its rounding can show (gsx_blend.hip: kKindRefOrder, blend_tile16_ref_kernel)
//   other semantics:
//     a = (x_pix, y_pix, Q''00, Q''01 + Q''10)   b = (Q''11, log2(opacity factor) | opacity, r, g)   c = (b, depth, 0, -)
struct __attribute__((aligned(16))) Record {
    float4 a, b, c;
};
static_assert(sizeof(Record) == kRecordBytes, "gsx_plan.h sizes the workspace with this");

// Tile rectangle of one Gaussian, inclusive, already clamped to the window; empty when x0 > x1.
struct TileRect {
    uint16_t x0, x1, y0, y1;
};
static_assert(sizeof(TileRect) == kTileRectBytes && sizeof(float4) == kBboxBytes && sizeof(uint2) == kRangeBytes,
              "gsx_plan.h sizes the workspace with these");

// ---- device helpers of more than one translation unit
// Tiles a rectangle covers: the pairs the emission writes for it (gsx_binning.hip, gsx_backward.hip).
__device__ __forceinline__ uint32_t tiles_of(const TileRect &r) {
    return r.x0 > r.x1 ? 0u : (uint32_t)(r.x1 - r.x0 + 1) * (uint32_t)(r.y1 - r.y0 + 1);
}

// min(*n_dev, bound), or bound when n_dev == nullptr: an element count that lives on the device (gsx_binning.hip, gsx_sort.hip).
__device__ __forceinline__ uint32_t load_count(const uint32_t *n_dev, uint32_t bound) {
    if (!n_dev) return bound;
    const uint32_t n = *n_dev;
    return n < bound ? n : bound;
}

// REF_CPU's stop rule: a pixel stops before the record that would take its transmittance below this (gaussian_scene.py:153).
constexpr float kStopRefCpu = 0.000001f;

// The reference's alpha of one pixel, operation for operation (splat/utils.py:357-365 as torch executes it,
// oracle/probe_torch_order.py; splat/gaussian_scene.py:164): d = -1/2 (mean - pixel) -- exact --, (1,2) @ (2,2) one FMA
// per output, the final (1,2) @ (2,1) two rounded products and a sum (every file is compiled with -ffp-contract=off),
// exp, times the opacity factor.  px, py: the pixel in FRAME coordinates (integers: exact as floats).  The exponential
// is v_exp_f32 of power * log2(e): within 2 ulp of expf plus 6e-8 |power| log2(e), i.e. < 2e-6 of alpha wherever
// alpha >= 1e-7 -- the one step that is not the reference's bit for bit.  The forward's compositing kernels
// (gsx_blend.hip) evaluate it; the kernels that walk the forward's lists evaluate alpha_ref_walk, below.
__device__ __forceinline__ float alpha_ref(float x, float y, float q00, float q01, float q10, float q11, float op,
                                           float px, float py) {
    const float e0 = x - px, e1 = y - py;
    const float d0 = -0.5f * e0, d1 = -0.5f * e1;
    const float t0 = __builtin_fmaf(d1, q10, d0 * q00);
    const float t1 = __builtin_fmaf(d1, q11, d0 * q01);
    const float power = t0 * e0 + t1 * e1;
    return __builtin_amdgcn_exp2f(power * 1.44269504088896340736f) * op;
}

// alpha_ref for the kernels that WALK the forward's lists (the backward's tile kernels, gsx_render_depth,
// gsx_render_contribution): the same operations up to `power`, the product power * log2(e) carried with its float32
// residual.  Rounding that product costs 6e-8 |power| log2(e) of alpha, which the frame cannot see but a gradient can: a
// Gaussian whose centre lies outside the rendered region is graded only on pixels several sigmas out, every term of its
// sums is off the same way, and dL/dopacity of such a row was 8.5e-7 of its error scale away from float64 (the reference's
// own float32 autograd: 3e-8).  p2 + lo is the product to 2^-48: lo = the product's own rounding error (one FMA) plus
// power times what float32 drops of log2(e); exp2(p2 + lo) = exp2(p2) (1 + lo ln 2) to 1e-14.  What is left is v_exp_f32's
// own 1 ulp, independent of |power|.
__device__ __forceinline__ float alpha_ref_walk(float x, float y, float q00, float q01, float q10, float q11, float op,
                                                float px, float py) {
    constexpr float kLog2e = 1.44269504088896340736f;
    constexpr float kLog2eLo = (float)(1.44269504088896340736 - (double)kLog2e);
    const float e0 = x - px, e1 = y - py;
    const float d0 = -0.5f * e0, d1 = -0.5f * e1;
    const float t0 = __builtin_fmaf(d1, q10, d0 * q00);
    const float t1 = __builtin_fmaf(d1, q11, d0 * q01);
    const float power = t0 * e0 + t1 * e1;
    const float p2 = power * kLog2e;
    const float lo = __builtin_fmaf(power, kLog2eLo, __builtin_fmaf(power, kLog2e, -p2));
    const float w = __builtin_amdgcn_exp2f(p2);
    // (outside v_exp_f32's range -- an overflowed or NaN exponent included -- the value is alpha_ref's: lo is inf - inf there)
    return (__builtin_fabsf(p2) < 126.0f ? __builtin_fmaf(w, lo * 0.693147180559945309417f, w) : w) * op;
}

// alpha_ref for the geometry moments.  v_exp_f32 returns zero where its result would be below 2^-126, so alpha_ref is
// exactly 0 for a pixel in the far tail of a footprint, where the reference's expf still returns 1e-38 .. 1e-45.  The
// frame and the colour sums cannot see the difference (T - T alpha == T, and T alpha c is below every sum's last bit
// unless the sum is itself that small); the moments of a Gaussian that is graded on such pixels ONLY consist of nothing
// else.  Below 2^-100 the exponential is taken 2^64 higher and scaled back after the opacity factor, one rounding into
// the subnormal range; elsewhere this is `alpha`, alpha_ref's own value.
__device__ __forceinline__ float alpha_ref_tail(float x, float y, float q00, float q01, float q10, float q11, float op,
                                                float px, float py, float alpha) {
    const float e0 = x - px, e1 = y - py;
    const float d0 = -0.5f * e0, d1 = -0.5f * e1;
    const float t0 = __builtin_fmaf(d1, q10, d0 * q00);
    const float t1 = __builtin_fmaf(d1, q11, d0 * q01);
    const float p2 = (t0 * e0 + t1 * e1) * 1.44269504088896340736f;
    return p2 < -100.0f ? (__builtin_amdgcn_exp2f(p2 + 64.0f) * op) * 0x1p-64f : alpha;
}

// GSX_SEM_STD_3DGS, one (pixel, Gaussian) pair: the exponent in log2 units from the packed record (x, y, Q''00, Qs'',
// Q''11), the rule set's two constants and its three decisions.  The forward's compositing kernels (gsx_blend.hip:
// std_composite) and the backward's std instances (gsx_backward_tile.inc) evaluate these same operations, so the set of
// composited pairs is one set.
constexpr float kStdAlphaMin = 1.0f / 255.0f, kStdStop = 0.0001f, kStdAlphaMax = 0.99f;

__device__ __forceinline__ float std_exponent(float e_x, float e_y, float Q00, float Qs, float Q11) {
    return __builtin_fmaf(e_y, __builtin_fmaf(e_y, Q11, e_x * Qs), (e_x * e_x) * Q00);
}

// `thr`: the pixel's alpha threshold, 1/255 while it is live.  use: neither skip rule applies; ta = T alpha; stop: the
// pixel ends BEFORE this pair.
__device__ __forceinline__ void std_tests(float pw, float alpha, float thr, float T, float &ta, bool &use, bool &stop) {
    use = !(pw > 0.0f) && !(alpha < thr);
    ta = T * alpha;
    stop = use && (T - ta < kStdStop);
}

// GSX_FLAG_ANTIALIASED (GSX_SEM_STD_3DGS): the opacity compensation of one Gaussian from its EWA covariance (ca0, cb, cd0)
// as ewa_covariance leaves it, BEFORE the 0.3 dilation, and det1, the determinant project_std forms AFTER it (the one its
// conic divides by).  rho = sqrt(max(0.000025, det0 / det1)); where the ratio does not exceed the floor -- a float32
// det0 <= 0 and a NaN included -- rho is the constant 0.005 and carries no gradient (clamped).  Stage 1 (gsx_project.hip:
// project_std) and the backward chain (gsx_backward.hip: geometry_chain) both call this on the same float32 values, so both
// take the same branch; every file is compiled with -ffp-contract=off: two rounded products, one difference, one quotient.
constexpr float kStdAaFloor = 0.000025f;
struct StdAaFactor {
    float det0, rho;
    bool clamped;
};
__device__ __forceinline__ StdAaFactor std_aa_factor(float ca0, float cb, float cd0, float det1) {
    StdAaFactor f;
    f.det0 = ca0 * cd0 - cb * cb;
    const float ratio = f.det0 / det1;
    f.clamped = !(ratio > kStdAaFloor);
    f.rho = f.clamped ? 0.005f : sqrtf(ratio);    // (sqrtf(fmaxf(0.000025f, ratio)), its floor spelled as the constant it is)
    return f;
}
// sigmoid(logit) as GSX_SEM_STD_3DGS's stage 1 forms it (gsx_project.hip: sigmoidf, the same operations): the anti-aliased
// record holds sigmoid(logit) * rho, and dL/dlogit needs the first factor alone.
__device__ __forceinline__ float std_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }

// Tiles whose list is much longer than the frame's average are composited by FOUR waves (a quarter of the
// tile's pixels each, one pixel per lane, eight records per trip) instead of one: a lone wave walks its list
// at ~430 cycles per record, so one 20 000-entry tile would outlast the rest of the frame several times over.
// The list of such tiles is built on the device by tile_ranges_kernel (count: zeroed by the emit kernel) and
// flagged in bit 31 of ranges[t].y; the compositing launch carries 4 * kMaxLongTiles helper workgroups.
constexpr uint32_t kLongFlag = 0x80000000u;
struct LongTiles {
    uint32_t *count;   // number of long tiles found (may exceed max)
    uint32_t *list;    // window-local tile ids, max entries
    uint32_t max;      // 0: the split is off for this frame
    // When the previous frame of the view left its tiles' costs (GsxParams.hints; header[kHintLens] and
    // header[kHintSched] name this window) a tile is long when it COST more than cost_pct % of a SIMD's share of the
    // frame (sum of all costs / 1024) -- see tile_ranges_kernel; cost == nullptr: by list length alone.
    uint32_t *cost = nullptr;
    const uint32_t *header = nullptr;
    uint32_t cost_pct = 30;
    // A tile that WAS long stays long down to stay_pct % of the threshold: four quarters (each walks its own block's list)
    // and one wave (the longest of four block lists per batch) do not report the same cost, and a tile within that
    // difference of the threshold changed sides on every frame -- nine tiles of the heavy-tailed test scene, whose frames
    // alternated between 0.476 and 0.556 ms (round 6, tools/frame_sequence.py).
    uint32_t stay_pct = 75;
    // one word, zeroed by the emit kernel: tiles and long-tile quarters of the tile-16 REF_CPU compositing launch that met a
    // reference-order record (GsxFrameStats.n_redo; with GSX_FLAG_PLAIN_FOOTPRINTS: that were left undone for it)
    uint32_t *redo = nullptr;
};
__host__ __device__ inline uint32_t long_tile_threshold(uint32_t pairs, uint32_t tiles) {
    const uint32_t mean = tiles ? pairs / tiles : 0u;
    const uint32_t four = mean > 0x3FFFFFFFu ? 0xFFFFFFFFu : 4u * mean;
    return four > 1024u ? four : 1024u;
}

struct StageOneOut {  // PreprocessedScene arrays (splat/schema.py:13-25), depth-sorted
    float *points_xy, *colors, *cov2d, *depths, *inv_cov, *radius, *min_x, *max_x, *min_y, *max_y, *sig_op;
    int32_t *order;
};

struct GaussiansIn {  // splat/gaussians.py:19-33
    const float *means3d, *scales, *quats, *opacity_logit, *colors;
    // GsxParams.original_index (or null): row i holds the Gaussian of that ORIGINAL index -- keys, records and rectangles
    // are filed under it (launch_project_pack pre-fills the keys with kEmptyKey first)
    const int32_t *original_index = nullptr;
    const float4 *block_bounds = nullptr;      // GsxParams.block_bounds (two float4 per GSX_BOUNDS_ROWS rows), or null
};

struct PreprocessedIn {  // argument list of splat/c/render.cu:90-101
    const float *means, *colors, *inv_cov, *min_x, *max_x, *min_y, *max_y, *opacity;
};

// The projection launch's share: one spare workgroup puts the compositing schedule of THIS frame together from the
// tiles' costs the previous frame left (gsx_schedule_device.h; sched == nullptr: not wanted).
struct ScheduleHint {
    const uint32_t *lens;
    uint32_t *sched, *header;
    uint32_t ntiles, nwy;       // tiles of the window, and along its y axis (tile ids are column-major)
};

// ---- gsx_project.hip (compiled with -ffp-contract=off)
// gsx_preprocess, first kernel: depth keys in original order (kCulledKey behind the cull plane), the 11 floats of
// every visible Gaussian that the rank-ordered output kernel gathers (in its record slot), the sort's counters zeroed.
// visible_rows: 0 = as many of the n Gaussians are visible as n suggests (the default), 1 = GSX_FLAG_ONE_VISIBLE,
// 2 = GSX_FLAG_SMALL_BATCH (two or three): which of its BLAS's orders the reference's products over the VISIBLE rows take.
hipError_t launch_project_stage(const GsxCamera &cam, const GaussiansIn &in, int64_t n, uint32_t *keys, Record *stage,
                                uint32_t *counters, int visible_rows, hipStream_t s);
// Original order: depth keys (kCulledKey behind the cull plane, kEmptyKey when no tile of the window is
// reached), records / rects indexed by the ORIGINAL Gaussian index (only written for the Gaussians that
// reach a tile; the depth sort generates the identity values itself).
// bbox (REF_CUDA only, else may be null): (min_x, max_x, min_y, max_y) per Gaussian for the
// per-pixel cull of splat/c/render.cu:55-60.
// tight_rects: GSX_SEM_STD_3DGS without GSX_FLAG_PUBLISHED_RECTS (see include/gsx.h).
// antialiased: GSX_FLAG_ANTIALIASED (GSX_SEM_STD_3DGS): the record's opacity is sigmoid(logit) * rho (std_aa_factor).
// cam_device (may be null): GsxParams.camera_device, read by the kernel instead of `cam`.
// sh_degree >= 0: in.colors holds spherical-harmonics coefficients, evaluated inline (GsxParams.sh).
// counters: 4 words this kernel zeroes for the depth sort (culled count, kept count, ...).
// A frame without splitters from an earlier frame of its view: `wgs` spare workgroups of the projection launch rank a sample
// of `ns` keys they compute themselves (gsx_sample_device.h) into the partition pass' splitters and zero its chunk sums --
// what sample_rank_kernel would do BEHIND the projection.  splitters == nullptr: not wanted.  (depth_presample, below: gsx_sort.hip)
struct SampleHint {
    uint32_t *splitters = nullptr;
    unsigned long long *chunk_sums = nullptr;
    uint32_t nsums = 0, ns = 0;
    const uint32_t *row_of = nullptr;      // GsxParams.row_of_index: sample index (an original index) -> row
};
hipError_t launch_project_pack(const GsxCamera &cam, const GsxCamera *cam_device, const GaussiansIn &in, int64_t n,
                               const TileGrid &grid, int semantics, bool tight_rects, bool antialiased, int visible_rows, int sh_degree,
                               uint32_t *keys, Record *rec, TileRect *rect, uint32_t *counters, float4 *bbox,
                               const ScheduleHint &sched, uint8_t *block_scratch, hipStream_t s,
                               const SampleHint &sample = SampleHint());
// (block_scratch: ceil(n / GSX_BOUNDS_ROWS) bytes the launch may use when in.block_bounds is set -- the depth sort's
// temp area, idle until the projection is done; in.original_index: the launch pre-fills the keys itself)
// gsx_preprocess, last kernel: all PreprocessedScene fields in depth order; order[r] = Gaussian of rank r, r < *m_dev.
hipError_t launch_project_full(const Record *stage, const uint32_t *order, const uint32_t *m_dev, int64_t n,
                               const StageOneOut &out, hipStream_t s);
hipError_t launch_pack_preprocessed(const PreprocessedIn &in, int64_t n, const TileGrid &grid, int semantics,
                                    Record *rec, TileRect *rect, float4 *bbox, hipStream_t s);
// The backward pass: per row, (x, y, Q00, Q01), (Q10, Q11, op, sigmoid(logit)), (r, g, b, radius) -- project_raw_kernel.
hipError_t launch_project_raw(const GsxCamera &cam, const GaussiansIn &in, int64_t n, int visible_rows, Record *raw, hipStream_t s);
// The view-space depth of every row, row4_view(p, world2view, 2, vis): the value project_raw_kernel builds its record on
// and the depth order its key (the reference's points_view[:, 2], PreprocessedScene.depths), same operations, same bits.
hipError_t launch_project_depth(const GsxCamera &cam, const float *means3d, int64_t n, int visible_rows, float *zrow, hipStream_t s);
hipError_t launch_covariance3d(const float *scales, const float *quats, int64_t n, float *out, hipStream_t s);
hipError_t launch_covariance2d(const GsxCamera &cam, const float *points, const float *cov3d, int64_t n, float *out,
                               hipStream_t s);
hipError_t launch_project_points(const GsxCamera &cam, const float *means3d, int64_t n, float *points_out,
                                 uint8_t *in_view, hipStream_t s);

// ---- gsx_binning.hip
// Where a frame's counts go on the device (and, optionally, straight into pinned host memory).
struct BinCounts {
    int64_t *stats2;             // [0] = visible Gaussians, [1] = D, [2] = Gaussians kept by the depth sort
    int64_t *stats2_host;        // device-visible alias of a pinned GsxFrameStats (fields 0, 1 and n_kept), or null
    uint32_t *d32;               // min(D, 2^32 - 1): element count of the tile sort
    uint32_t *long_count;        // zeroed by the emit kernel for tile_ranges_kernel (LongTiles.count)
    uint32_t *redo_count;        // zeroed by the emit kernel for the compositing launch (LongTiles.redo[0])
    const uint32_t *culled_dev;  // Gaussians behind the cull plane (counted by the depth sort), or null
    int64_t n_total;             // n_visible = n_total - *culled_dev
};
// One (tile id, Gaussian index) pair per covered tile, in rank order, from the rank-ordered tile
// rectangles rrect[0 .. m) (m = min(*m_dev, n); m_dev == nullptr: n).  order[r] = Gaussian index of rank
// r (nullptr: the identity).  Also zeroes ranges[] and delivers the frame's counts (bc).  keys0 / vals0
// hold cap 32-bit words each; pairs beyond cap are dropped.  sums_ready: emit_chunk_sums(temp, n, cap) already
// holds the chunk sums (the sampled depth sort left them there).
hipError_t emit_instances(void *temp, const TileRect *rrect, const uint32_t *order, const uint32_t *m_dev, int64_t n,
                          int64_t cap, const TileGrid &grid, void *keys0, uint32_t *vals0, uint2 *ranges,
                          const BinCounts &bc, bool sums_ready, int64_t kept_hint, hipStream_t s);
// Stable sort of the emitted pairs by tile id and ranges[t] = [first, last) for every tile of the
// window; *sorted_vals points at the sorted Gaussian indices.  The pair count is read from *d32.
hipError_t sort_instances(void *temp, int64_t cap, const TileGrid &grid, void *keys0, void *keys1, uint32_t *vals0,
                          uint32_t *vals1, uint2 *ranges, const uint32_t *d32, const LongTiles &lt,
                          const uint32_t **sorted_vals, hipStream_t s);
// counts[t] = length of tile t's list (GsxParams.tile_counts).
hipError_t launch_tile_counts(const uint2 *ranges, int64_t nt, uint32_t *counts, hipStream_t s);
// sched[k] = tile with the k-th longest list (1024 length classes), for launch_blend's balanced hand-out.
hipError_t launch_tile_schedule(const uint2 *ranges, int64_t nt, uint32_t *sched, hipStream_t s);
// the per-XCD schedule of THIS frame's list lengths (REF_CPU tile 16; header: kHintHeaderWords words, sched: hints_sched_entries)
hipError_t launch_tile_schedule_xcd(const uint2 *ranges, int64_t nt, int64_t nwy, uint32_t *sched, uint32_t *header, hipStream_t s);
// ---- gsx_sort.hip: stable LSD radix sort, up to 8 bits per pass, key bits [0, key_bits).  The element
// count is min(*n_dev, bound) (n_dev == nullptr: bound); grids are sized by `bound`.  Buffers
// ping-pong; on return keys_cur / vals_cur point at the sorted data.  temp: radix_temp_bytes(bound).
hipError_t radix_sort_pairs_u32(void *temp, uint32_t *&keys_cur, uint32_t *&keys_alt, uint32_t *&vals_cur,
                                uint32_t *&vals_alt, const uint32_t *n_dev, int64_t bound, int key_bits,
                                hipStream_t s);
hipError_t radix_sort_pairs_u16(void *temp, uint16_t *&keys_cur, uint16_t *&keys_alt, uint32_t *&vals_cur,
                                uint32_t *&vals_alt, const uint32_t *n_dev, int64_t bound, int key_bits,
                                hipStream_t s);
// Depth sort of the whole-path entry point: all 32 key bits, dropping keys >= kEmptyKey in the first
// pass (*m_dev = Gaussians kept, *culled_dev += keys == kCulledKey; culled_dev must hold 0 when the
// first kernel runs) and gathering rect[index] into rrect[rank] in the last one.  On return
// vals_cur[0 .. *m_dev) = Gaussian index of each depth rank (ties: original index).  The values of the
// first pass are the item positions themselves (vals_cur need not be initialised).
// row_of (both depth sorts; or null): GsxParams.row_of_index -- the keys are filed under ORIGINAL indices, the value an item
// gets in the first pass is the ROW that index names (records and rectangles are in row order)
hipError_t sort_depth_compact(void *temp, uint32_t *keys0, uint32_t *keys1, uint32_t *&vals_cur, uint32_t *&vals_alt,
                              int64_t n, uint32_t *m_dev, uint32_t *culled_dev, const TileRect *rect, TileRect *rrect,
                              hipStream_t s, uint32_t *samples_out = nullptr, uint32_t *carry0 = nullptr,
                              uint32_t *carry1 = nullptr, const uint32_t *row_of = nullptr);

// The same contract with 5 kernels instead of 12: sample 2048 / 8192 keys -> 255 / 1023 splitters, ONE stable
// partition pass, one in-LDS sort per bucket (gsx_sort.hip).  depth_sort_route picks the route from the
// Gaussian count and the caller's hint of how many of them reach a tile (GsxParams.kept_hint; 0 = unknown).
// lds_cap: 0 = the bucket kernel's capacity; tests pass a small value to drive buckets through its global-memory path.
enum DepthRoute { kDepthLsd = 0, kDepth256 = 1, kDepth1024 = 2, kDepthOneWorkgroup = 3 };
DepthRoute depth_sort_route(int64_t n, int64_t kept_hint);
SampleHint depth_presample(DepthRoute route, void *temp, int64_t n, uint64_t *chunk_sums, const uint32_t *row_of);
// The depth sort's share of GsxParams.hints (gsx_plan.h: hints_layout); header == nullptr: no hints buffer.
struct SortHints {
    uint32_t *header;           // kHintSplitters says whether `splitters` are there, kHintLens / kHintSched how many tiles
    const uint32_t *splitters;  // 256 words left by the previous frame
    uint32_t *samples;          // kSortSamples words this frame's count kernel fills for the next frame
    bool use;                   // GSX_FLAG_HINTS_VALID: partition with `splitters`, no sample kernel
    // the 256-bucket route (round 6): the bucket kernel knows every kept key's rank and leaves the NEXT frame's splitters
    // itself -- the EXACT 256-quantiles of this frame's keys, in place of the hints' splitters (every reader of the current
    // ones has finished) -- instead of a sample for the compositing launch's spare workgroups to rank; null: not wanted
    uint32_t *next_splitters = nullptr;
};

// The compositing launch's share: spare workgroups rank the samples into the next frame's splitters, every tile
// workgroup leaves the length of its list.  header == nullptr: no hints buffer.
struct BlendHints {
    uint32_t *header;
    const uint32_t *samples;    // kSortSamples words of this frame's count kernel, or nullptr (nothing to rank)
    uint32_t *splitters;
    uint32_t *lens;
    uint32_t xcd_sched;         // != 0: `sched` is hints.sched, the per-XCD schedule (gsx_schedule_device.h) -- trusted
                                // only if header[kHintSched] == number of tiles; 0: tile_schedule_kernel's whole-frame order
    uint32_t rank_last = 0;     // the spare workgroups that rank the samples come last in the grid instead of first
    uint32_t plain = 0;         // GSX_FLAG_PLAIN_FOOTPRINTS: the compositing instance that cannot evaluate reference-order records
};
hipError_t sort_depth_sampled(DepthRoute route, void *temp, uint32_t *keys0, uint32_t *keys1, uint32_t *&vals_cur,
                              uint32_t *&vals_alt, int64_t n, int64_t kept_hint, uint32_t *m_dev, uint32_t *culled_dev,
                              const TileRect *rect, TileRect *rrect, uint32_t lds_cap, uint64_t *chunk_sums,
                              const SortHints &hints, hipStream_t s, const uint32_t *row_of = nullptr, bool presampled = false);
// Where emit_instances keeps its chunk sums inside `temp` (for sort_depth_sampled to fill them in).
uint64_t *emit_chunk_sums(void *temp, int64_t n, int64_t cap);

// ---- gsx_sh.hip
hipError_t launch_sh_to_rgb(const float *means3d, const float *sh, int degree, int64_t n, const float *center,
                            float *colors, hipStream_t s);
// dL/dcolors (n,3) -> dL/dsh (n,K,3), every entry written, and (grad_means3d may be NULL) dL/dmeans3d (n,3) through the view
// direction, written, not accumulated.  A degree outside 0..3: hipErrorInvalidValue.
hipError_t launch_sh_backward(const float *means3d, const float *sh, int degree, int64_t n, const float *center,
                              const float *grad_colors, float *grad_sh, float *grad_means3d, hipStream_t s);

// ---- gsx_sh_active.hip
// The two above on the first (active+1)^2 coefficients of rows stored at degree `stored` (sh, grad_sh: (n, (stored+1)^2, 3)):
// the bits of the packed degree-`active` call; the tail of every grad_sh row is written +0.  active == stored: the two above.
// Degrees outside 0..3 or active > stored: hipErrorInvalidValue.
hipError_t launch_sh_to_rgb_active(const float *means3d, const float *sh, int stored, int active, int64_t n,
                                   const float *center, float *colors, hipStream_t s);
hipError_t launch_sh_backward_active(const float *means3d, const float *sh, int stored, int active, int64_t n,
                                     const float *center, const float *grad_colors, float *grad_sh, float *grad_means3d,
                                     hipStream_t s);

// ---- gsx_loss.hip
// gsx_photometric_loss behind its argument checks: loss_out = (loss, l1, ssim) over the rows x cols region and, when
// grad_image is not NULL, dloss/dimage into it.  `ws` is carved by `c` (plan::loss_carve with with_grad = grad_image != NULL).
struct LossImages {
    const float *image, *target;
    float *grad;                       // or NULL
    int64_t image_stride, target_stride, grad_stride;   // floats per row
    int32_t rows, cols;
};
hipError_t launch_photometric_loss(const LossImages &im, float lambda, float *loss_out, char *ws, const plan::LossCarve &c,
                                   hipStream_t s);

// ---- gsx_loss_weighted.hip
// gsx_photometric_loss_weighted behind its argument checks, with a weight or an exposure (with neither the entry calls
// launch_photometric_loss and launch_loss_weight_sum): loss_out = (loss, l1, ssim, W); dloss/dimage when im.grad, dloss/dE
// when grad_exposure.  `ws` is carved by `c` (plan::loss_weighted_carve with with_grad = im.grad != NULL).
struct LossWeights {
    const float *weight;               // DEVICE (rows x cols), a row every weight_stride floats, or NULL: all ones
    int64_t weight_stride;
    const float *exposure;             // DEVICE 12 floats, row-major 3 x 4, or NULL: the identity
    float *grad_exposure;              // DEVICE 12 floats, or NULL
};
hipError_t launch_photometric_loss_weighted(const LossImages &im, const LossWeights &wt, float lambda, float *loss_out, char *ws,
                                            const plan::LossWeightedCarve &c, hipStream_t s);
// loss_out[3] = rows * cols, what W is without a weight.
hipError_t launch_loss_weight_sum(int32_t rows, int32_t cols, float *loss_out, hipStream_t s);

// ---- gsx_adam.hip
// gsx_adam_step behind its argument checks.  One workgroup per kAdamRows rows; the whole struct is the kernel's argument.
constexpr int kAdamRows = 256;
constexpr int kAdamMaxWidth = 1 << 20;      // a block's run of a group, kAdamRows * width floats, is indexed with 32 bits
struct AdamGroupArgs {
    float *param;
    const float *grad;
    float *exp_avg, *exp_avg_sq;
    int32_t width;
    int32_t log_space;      // GSX_ADAM_LOG
    float a;                // lr / (1 - beta1^step)
    int32_t vec;            // all four bases are 16-byte aligned
};
struct AdamArgs {
    AdamGroupArgs group[8];
    int64_t n;
    int32_t n_groups;
    float beta1, beta2, c1, c2, s2, eps;    // c1 = 1 - beta1, c2 = 1 - beta2, s2 = sqrt(1 - beta2^step)
};
hipError_t launch_adam(const AdamArgs &args, bool skip_zero_rows, hipStream_t s);

// ---- gsx_transform.hip
// gsx_transform_gaussians behind its argument checks.  One workgroup per kTransformRows rows; the whole struct is the kernel's
// argument (the matrices are read with scalar loads).
constexpr int kTransformRows = 256;             // kAdamRows, sh::kBlock, block_bounds
struct TransformArgs {
    float *points, *scales, *quats, *sh;        // sh: nullptr when degree == 0
    int64_t n;
    int32_t vec;                                // sh is 16-byte aligned
    GsxTransform T;
};
hipError_t launch_transform(const TransformArgs &args, int degree, hipStream_t s);

// ---- gsx_rectify.hip
// gsx_rectify_photo behind its argument checks.  One thread per output pixel, kRectifyJ along the output's contiguous axis j
// by kRectifyI along i; the whole struct is the kernel's argument.  k1, k2, p1, p2: the lens model's coefficients, zero where
// the model has none (a pinhole is the OPENCV body with four zeros: the same operations, exact).
constexpr int kRectifyJ = 8, kRectifyI = 32;
constexpr int kRectifyMaxSize = 1 << 16;        // of either image, per axis
struct RectifyArgs {
    const uint8_t *photo;
    int64_t row_stride;
    float *image, *weight;                      // weight: or null
    int32_t src_w, src_h, out_w, out_h, samples;
    float fxs, fys, cxs, cys, k1, k2, p1, p2;   // the photo's camera
    float fx, fy, cx, cy;                       // the target, in output index coordinates
};
hipError_t launch_rectify(const RectifyArgs &args, hipStream_t s);

// ---- gsx_density.hip
// gsx_density_accumulate / _plan / _apply behind their argument checks.  The workspace of n rows (DensityCarve):
//   header  kDensityHeader bytes: int64 n, n_out, n_pruned, n_cloned, n_split; float split_shrink at kDensityShrinkAt
//   action  one byte per row (kDensityKeep ..), padded to whole scan blocks of kDensityScanRows rows
//   prefix  uint32 per row: the row's first output row
//   bsum    per scan block (+1): the output rows of the blocks before it; then the blocks' pruned and split counts
constexpr int kDensityRows = 256;               // source rows of one workgroup of the apply kernel (kAdamRows, block_bounds)
constexpr int kDensityScanRows = 1024;          // rows of one workgroup of the plan's scan
constexpr int kDensityScanPass = 256 * kDensityScanRows;    // rows one pass of the block-level scan covers
constexpr int64_t kDensityMaxRows = (int64_t)1 << 30;
constexpr int kDensityMaxWidth = 1 << 20;       // a block's run of a group, at most 512 * width floats, is indexed with 32 bits
constexpr size_t kDensityHeader = 256, kDensityShrinkAt = 40;
enum : uint8_t { kDensityKeep = 0, kDensityPrune = 1, kDensityClone = 2, kDensitySplit = 3 };
struct DensityCarve {
    size_t action, prefix, bsum, total;
    uint32_t scan_blocks;
};
inline bool density_carve(int64_t n, DensityCarve &c) {
    if (n < 0 || n > kDensityMaxRows) return false;
    const size_t nsb = (size_t)((n + kDensityScanRows - 1) / kDensityScanRows);
    const auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    c.scan_blocks = (uint32_t)nsb;
    c.action = kDensityHeader;
    c.prefix = c.action + up(nsb * kDensityScanRows);
    c.bsum = c.prefix + up((size_t)n * 4);
    c.total = c.bsum + up((3 * nsb + 1) * 4);
    return true;
}
struct DensityGroupArgs {
    const float *src;
    float *dst;
    int32_t width, role;
};
struct DensityArgs {
    DensityGroupArgs group[24];
    const float *scales, *quats, *noise;    // the POINTS group's companions (null without one)
    const uint8_t *action;
    const uint32_t *prefix;
    int32_t *source_row;                    // or null
    const float *shrink;                    // rules.split_shrink, where the plan left it in the header
    int64_t n;
    int32_t n_groups;
};
hipError_t launch_density_accumulate(const float *grad, int32_t width, int64_t n, float *grad_sum, uint32_t *seen, hipStream_t s);
hipError_t launch_density_plan(const float *grad_sum, const uint32_t *seen, const float *scales, const float *opacity_logit,
                               int64_t n, const GsxDensityRules &rules, char *ws, const DensityCarve &c, hipStream_t s);
hipError_t launch_density_apply(const DensityArgs &args, int64_t n_out, hipStream_t s);
// what launch_density_plan runs behind its classify kernel: the scan of the block sums with the header, then every row's
// first output row (the action bytes and the three per-block counts are in `ws` by then)
hipError_t launch_density_plan_finish(int64_t n, float split_shrink, char *ws, const DensityCarve &c, hipStream_t s);

// ---- gsx_density_screen.hip
// gsx_density_accumulate_screen / gsx_density_plan_screen behind their argument checks.  The plan's workspace is
// gsx_density_plan's (radius_max may be null: the same bytes).
hipError_t launch_density_accumulate_screen(const float *grad_means2d, const float *screen_radius, int64_t n, float *grad_sum,
                                            uint32_t *seen, float *radius_max, hipStream_t s);
hipError_t launch_density_plan_screen(const float *grad_sum, const uint32_t *seen, const float *scales, const float *opacity_logit,
                                      const float *radius_max, float prune_radius, int64_t n, const GsxDensityRules &rules,
                                      char *ws, const DensityCarve &c, hipStream_t s);

// ---- gsx_mcmc.hip
// gsx_mcmc_regularize / _perturb / _plan / _apply behind their argument checks.  The plan's workspace: plan::McmcCarve.
constexpr int kMcmcRows = 256;                  // output rows of one workgroup of the apply kernel (kDensityRows, kAdamRows)
constexpr int kMcmcMaxWidth = 1 << 20;          // a block's run of a group, 256 * width floats, is indexed with 32 bits
struct McmcRegularizeArgs {
    const float *opacity, *scales;
    float *grad_opacity, *grad_scales;          // null: that side is off (its lambda is 0)
    int64_t n;
    float coef_opacity, coef_scale;             // lambda_opacity / n, lambda_scale / (3 n): in double, rounded to float
    int32_t vec;                                // every base in use is 16-byte aligned
};
struct McmcPerturbArgs {
    float *points;
    const float *scales, *quats, *opacity, *noise;
    int64_t n;
    float rate, gate_k, gate_x0;
    int32_t vec;
};
struct McmcPlanArgs {
    const float *opacity;
    const double *uniforms;
    uint32_t *weights, *count;
    int32_t *source;
    int64_t n, n_out;
    float dead_logit;
};
struct McmcApplyArgs {
    DensityGroupArgs group[24];                 // role: GSX_MCMC_COPY ..
    const int32_t *source;
    const uint32_t *count;
    const float *opacity;                       // the OPACITY group's src, or null without one
    int64_t n, n_out;
    int32_t n_groups;
    float min_opacity;
};
hipError_t launch_mcmc_regularize(const McmcRegularizeArgs &args, hipStream_t s);
hipError_t launch_mcmc_perturb(const McmcPerturbArgs &args, hipStream_t s);
hipError_t launch_mcmc_plan(const McmcPlanArgs &args, char *ws, const plan::McmcCarve &c, hipStream_t s);
hipError_t launch_mcmc_apply(const McmcApplyArgs &args, hipStream_t s);

// ---- gsx_knn.hip
// gsx_knn3 behind its argument checks.  The workspace of n rows (KnnCarve):
//   header  kKnnHeader bytes: uint64 (query, candidate) pairs evaluated (zeroed and read only when the caller asks)
//   boxes   two float4 per block of kKnnRows consecutive entries: (min xyz, 0), (max xyz, 0)
//   pts     float4 per entry: (x, y, z, the bits of the entry's row), in the caller's `order`
constexpr int kKnnRows = 256;                   // entries of one workgroup (kAdamRows, kDensityRows, block_bounds)
constexpr int64_t kKnnMaxRows = (int64_t)1 << 30;
constexpr size_t kKnnHeader = 256;
struct KnnCarve {
    size_t boxes, pts, total;
    uint32_t blocks;
};
inline bool knn_carve(int64_t n, KnnCarve &c) {
    if (n < 0 || n > kKnnMaxRows) return false;
    const size_t nb = (size_t)((n + kKnnRows - 1) / kKnnRows);
    const auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    c.blocks = (uint32_t)nb;
    c.boxes = kKnnHeader;
    c.pts = c.boxes + up(nb * 32);
    c.total = c.pts + up((size_t)n * 16);
    return true;
}
// counter: the header's uint64, or nullptr when nobody asked
hipError_t launch_knn3(const float *points, int64_t n, const int32_t *order, int32_t rule, float *dist3, float *scale,
                       char *ws, const KnnCarve &c, bool count, hipStream_t s);

// ---- gsx_blend.hip
// background: 3 floats, read on the host (GSX_SEM_STD_3DGS only); generic: GSX_FLAG_GENERIC_KERNELS.
// cp: what the launch zeroes besides compositing its tiles (extra workgroups of the same kernel).
// lt: long tiles split over four waves (GSX_SEM_REF_CPU, tile 16 only; lt.max == 0 otherwise).
// sched: launch_tile_schedule's order, or nullptr (tiles in index order); used by the tile-16 REF_CPU kernel.
// asked: Plan.schedule (1 / 0 from the caller's flags, -1: by the size of the scene).
bool blend_uses_schedule(const TileGrid &grid, int semantics, bool generic, int64_t n, int asked);
// One part of the window (GsxParams.n_substrips): the tiles whose column (axis 0) / row (axis 1) -- absolute tile
// coordinate -- lies in [lo, hi); first: this launch also does what a frame does once (zero fill, next frame's splitters).
struct TileSpan {
    int32_t axis, lo, hi;
    uint32_t first;
    uint32_t index = 0;         // which part (0 .. 15)
};
// can this kernel family composite a window in parts?  (tile-16 REF_CPU kernel only; the others take one launch)
bool blend_in_parts(const TileGrid &grid, int semantics, bool generic);
// part: nullptr = the whole window in one launch
hipError_t launch_blend(const Record *rec, const float4 *bbox, const uint32_t *sorted_vals, const uint2 *ranges,
                        const TileGrid &grid, const OutDesc &out, int semantics, const float *background,
                        bool generic, const ClearPlan &cp, const LongTiles &lt, const uint32_t *sched,
                        const BlendHints &hints, hipStream_t s, const TileSpan *part = nullptr);
bool blend_splits_long_tiles(const TileGrid &grid, int semantics, bool generic);
hipError_t launch_clear(const ClearPlan &cp, float *base, hipStream_t s);   // the zero fill alone
hipError_t launch_zero_words(uint32_t *p, size_t n, hipStream_t s);

// ---- gsx_backward.hip (GSX_SEM_REF_CPU): gradients of the frame with respect to the colours and opacity logits, and
// (gsx_render_backward_geometry) the points, scales and quaternions
// Exclusive scan of the tile counts of the rank-ordered rectangles rrect[0 .. m): prefix[r] = emission slot of rank r's
// first pair (gsx_binning.hip emits a Gaussian's pairs over its rectangle, column by column), prefix[m] = D.  Also
// rank_of[order[r]] = r.  bsum: one word per 1024 ranks (+1).
hipError_t launch_backward_prefix(const TileRect *rrect, const uint32_t *order, uint32_t m, uint32_t *prefix,
                                  uint32_t *rank_of, uint32_t *bsum, hipStream_t s);
struct BackwardTiles {
    const Record *raw;            // launch_project_raw, by row
    const uint32_t *vals;         // sorted pair list: row of each entry, tile by tile
    const uint2 *ranges;          // [first, last) of every window tile's list
    const uint32_t *rank_of, *prefix;
    const TileRect *rrect;
    const float *image, *grad_image;   // the forward's frame and dL/dframe, layout of `out`
    float4 *slots;                // one per pair, in emission order: (dL/dc rgb, sum over the tile of dL/dalpha * alpha)
    // gsx_render_backward_geometry (else null: the colour-only instance runs): two per pair, the moments of
    // u = dL/dalpha * alpha over the tile with d = mean - pixel: (sum u d0, u d1, u d0^2, u d0 d1), (sum u d1^2, 0, 0, 0)
    float4 *geo_slots = nullptr;
};
hipError_t launch_backward_tiles(const BackwardTiles &bt, const TileGrid &grid, const OutDesc &out, hipStream_t s);
// gsx_render_backward_screen_abs: the tile kernel's abs instance, bt as above with geo_slots set; the pair's second geometry
// float4 becomes (S5, 0, Tx, Ty), the sums over the tile's pixels of the absolute value of each pixel's term of
// (Q + Q^T) u d (gsx_backward_tile.inc).  launch_backward_geometry with grad_means2d_abs then sums them beside the moments.
hipError_t launch_backward_tiles_abs(const BackwardTiles &bt, const TileGrid &grid, const OutDesc &out, hipStream_t s);
// gsx_render_depth / gsx_render_backward_depth: the depth image holds (D, A) per pixel, D = sum T alpha z the expected
// depth and A = sum T alpha the coverage, with the frame's two leading axes and 2 floats where the frame has 3 -- the
// float index of frame pixel (px, py) in it, from the frame's descriptor (whose strides are multiples of 3):
__host__ __device__ inline int64_t depth_index(const OutDesc &o, int px, int py) {
    return ((int64_t)(px - o.x0) * (o.stride_x / 3) + (int64_t)(py - o.y0) * (o.stride_y / 3)) * 2;
}
struct DepthTiles {
    const float *zrow;            // launch_project_depth, by row: the view-space depth the depth order is built on
    const float *depth;           // gsx_render_depth's image (backward only)
    const float *grad_depth;      // dL/d(depth image), same layout (backward only)
};
// The tile kernel's depth instance: bt as for launch_backward_tiles with geo_slots set; the pair's second geometry float4
// becomes (S5, Sz, 0, 0), Sz = sum T alpha dL/dD = dL/dz of the record over the tile.
hipError_t launch_backward_tiles_depth(const BackwardTiles &bt, const DepthTiles &dt, const TileGrid &grid, const OutDesc &out,
                                       hipStream_t s);
// gsx_render_depth: one wave per window tile walks its list as the backward does (alpha_ref_walk, kStopRefCpu, every listed
// record) and writes (D, A) of every pixel of its tile.  raw, vals, ranges as in BackwardTiles.
hipError_t launch_depth_tiles(const Record *raw, const uint32_t *vals, const uint2 *ranges, const float *zrow,
                              const TileGrid &grid, const OutDesc &out, float *depth, hipStream_t s);
// ---- The per-Gaussian half, behind the tile kernels: every launch below takes what the walk left per depth rank and, where
// it runs the chain, the rows it reads and writes.
struct RankSlots {
    const float4 *slots;          // BackwardTiles::slots
    float4 *geo_slots;            // BackwardTiles::geo_slots, or null: the colour-only calls
    const uint32_t *prefix;       // launch_backward_prefix: rank r's pairs are slots [prefix[r], prefix[r + 1])
    const uint32_t *order;        // row of rank r
    uint32_t m;                   // ranks
};
struct GeometryRows {
    const float *means3d, *scales, *quats;                  // (n,3), (n,3), (n,4): stage 1's inputs
    float *grad_means3d, *grad_scales, *grad_quats;         // the same shapes, zeroed by the caller
    // gsx_render_backward_screen: (n,2) the chain's dL/d(NDC mean), and (n) the radius -- GSX_SEM_REF_CPU: the raw record's, or
    // null; GSX_SEM_STD_3DGS: the chain's own, both or neither.  Null: gsx_render_backward_geometry
    float *grad_means2d, *screen_radius;
};
struct CameraGrads {
    float *world2view, *full_proj;   // device, 16 floats each
    float *partials;                 // workspace
};
// The colour sums: slots of each rank summed in emission order (one wave per rank), the rule set's way from sum u to
// dL/dlogit applied -- raw: the sigmoid applied twice; rec, the PACKED records of the forward's own projection
// (a = (x, y, Q''00, Qs''), b = (Q''11, opacity, r, g), c.x = b): (sum u)(1 - op) --, scattered to rows (order[r]).
hipError_t launch_backward_sums(const RankSlots &rk, const Record *raw, float *grad_colors, float *grad_opacity_logit,
                                hipStream_t s);
hipError_t launch_backward_sums_std(const RankSlots &rk, const Record *rec, float *grad_colors, float *grad_opacity_logit,
                                    hipStream_t s);
// The geometry sums and the chain: geometry slots of each rank summed in emission order (one wave per rank; the sums are
// left in the rank's first slot pair), then one thread per rank runs the chain from dL/dQ and dL/dmean to the inputs
// (gsx_backward.hip: geometry_chain) and scatters to rows (order[r]).
// launch_backward_geometry: gsx_render_backward_geometry and _screen, and
//   gsx_render_backward_camera (cg not null): the chain kernel's camera instance also leaves each block's 24 terms of
//     dL/dworld2view and dL/dfull_proj in a row of cg->partials (kCameraPartialBytes per 256 ranks, gsx_plan.h), and one
//     small kernel adds the rows in a fixed order into the two 4x4 outputs;
//   gsx_render_backward_screen_abs (grad_means2d_abs not null, cg null; after launch_backward_tiles_abs): the sum kernel's abs
//     instance adds Tx and Ty beside the five moments, in emission order and a fixed butterfly, and stores
//     (0.5 Tx |sx|, 0.5 Ty |sy|) to the Gaussian's row of grad_means2d_abs (n,2), which the caller has zeroed.
// launch_backward_geometry_depth (gsx_render_backward_depth): the sixth sum Sz beside S5, in the same order, and the chain
//   adds Sz world2view[0:3][2] to dL/dpoint: z = p . world2view[:3][2] + world2view[3][2] (no camera terms).
// launch_backward_geometry_std (gsx_render_backward_std, after launch_backward_sums_std): the chain's std variant, which forms
//   conic and radius itself.
hipError_t launch_backward_geometry(const GsxCamera &camera, const RankSlots &rk, const Record *raw, const GeometryRows &rows,
                                    hipStream_t s, const CameraGrads *cg = nullptr, float *grad_means2d_abs = nullptr);
hipError_t launch_backward_geometry_depth(const GsxCamera &camera, const RankSlots &rk, const Record *raw,
                                          const GeometryRows &rows, hipStream_t s);
hipError_t launch_backward_geometry_std(const GsxCamera &camera, const RankSlots &rk, const GeometryRows &rows, hipStream_t s);
// gsx_render_backward_std's tile kernels, two std instances on the packed records (bt.raw = the frame's records; geo_slots
// null: the colour-only instance)
hipError_t launch_backward_tiles_std(const BackwardTiles &bt, const TileGrid &grid, const OutDesc &out, hipStream_t s);
// GSX_FLAG_ANTIALIASED: what the two std launches do on records that hold sigmoid(logit) * rho (std_aa_factor) -- the
// geometry sums, then the colour sums with dL/dlogit = (sum u)(1 - sigmoid(logit)) from the opacity input, which also hand
// sum u to the chain's anti-aliased variant through a free word of the Gaussian's first geometry slot pair.  rk.geo_slots
// null: the colour-only call (rows is not read, the five geometry outputs are not touched).
hipError_t launch_backward_std_antialiased(const GsxCamera &camera, const RankSlots &rk, const GeometryRows &rows,
                                           const float *opacity_logit, float *grad_colors, float *grad_opacity_logit,
                                           hipStream_t s);

// ---- gsx_contribution.hip (gsx_render_contribution): the gradient entries' walk with no image and no gradient
struct ContributionTiles {
    const Record *raw;            // GSX_SEM_REF_CPU: launch_project_raw, by row; GSX_SEM_STD_3DGS: the frame's packed records
    const uint32_t *vals;         // sorted pair list: row of each entry, tile by tile
    const uint2 *ranges;          // [first, last) of every window tile's list
    const uint32_t *rank_of, *prefix;
    const TileRect *rrect;
    float4 *slots;                // one per pair, in emission order: (max T alpha, sum T alpha, bits of the pixel count, 0)
};
hipError_t launch_contribution_tiles(const ContributionTiles &ct, const TileGrid &grid, bool std_rules, hipStream_t s);
// slots of each rank reduced in emission order and written to row order[r] of the three arrays (views: or null), or --
// accumulate -- merged into it: max, +, +, views + 1
hipError_t launch_contribution_sums(const float4 *slots, const uint32_t *prefix, const uint32_t *order, uint32_t m,
                                    float *weight_max, float *weight_sum, uint32_t *pixels, uint32_t *views, bool accumulate,
                                    hipStream_t s);
// gsx_density_plan_contribution behind its argument checks (views may be null); the workspace is gsx_density_plan's
hipError_t launch_density_plan_contribution(const float *weight_max, const uint32_t *views, float threshold, int64_t n, char *ws,
                                            const DensityCarve &c, hipStream_t s);

}  // namespace gsx
