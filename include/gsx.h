/*
 * gsx.h -- C ABI of libgsx.so, the MI355X (gfx950) forward Gaussian-splat rasteriser.
 *
 * This is the drop-in boundary for the hot path of dcaustin33/intro_to_gaussian_splatting:
 * plain pointers and sizes, no torch types, no C++ exceptions.  Every entry point cites the
 * reference interface it replaces (paths relative to the reference repository).
 *
 * Conventions
 *   - All array pointers are DEVICE pointers to contiguous float32 (or the stated integer type)
 *     on the current HIP device, unless the name ends in `_host`.
 *   - All work is enqueued on `stream` (a hipStream_t passed as void*; NULL = default stream).
 *     Calls that report a host-side count (n_visible / n_instances) synchronise that stream
 *     once, after their last launch; nothing else blocks.
 *   - The library never allocates, frees or retains device memory: the caller owns inputs,
 *     outputs and the workspace (size from gsx_workspace_bytes).
 *   - Return value: GSX_OK (0) or a negative GsxStatus; gsx_last_error() gives a thread-local
 *     message for the last failing call on the calling thread.
 */
#ifndef GSX_H_
#define GSX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSX_VERSION 305 /* major*10000 + minor*100 + patch.  305: GsxParams.stats_size, .original_index, .block_bounds and .row_of_index (160 bytes): GsxFrameStats is written only as far
                         * as the caller says its struct reaches (64 bytes -- the ABI-300 struct, no n_redo -- when params is NULL or ends
                         * before the field); GSX_FLAG_PLAIN_FOOTPRINTS needs stats_size >= 72.  Binaries built against the 302 .. 304
                         * headers must be REBUILT (their 128-byte GsxParams is still read, but their 72-byte GsxFrameStats gets no
                         * n_redo, and a 302 binary that fills its struct through the exported function gsx_default_params has its
                         * n_substrips fields ignored -- see there).  304: one compositing launch; GSX_FLAG_SKIP_REDO (303) is now
                         * GSX_FLAG_PLAIN_FOOTPRINTS, same value and contract; gsx_hints_bytes is smaller.  303: GsxFrameStats.n_redo (72 bytes);
                         * gsx_default_params_sized (gsx_default_params is a macro over
                         * it; the exported function of that name serves ABI 300 / 301 binaries), GSX_FLAG_SMALL_BATCH / _ONE_VISIBLE,
                         * stage 1 in the operation order torch executes.  302: GsxParams.n_substrips .. substrip_events (appended;
                         * a struct_size of 104 -- or 0 -- still means the ABI-300 struct).  301: GsxParams.struct_size (in
                         * reserved0's place), a larger schedule region in gsx_hints_bytes.  300: GsxParams.kept_hint, GsxFrameStats.n_kept,
                           * tile_counts zeroed when nothing is rendered, tile_x1 == tile_x0 is an empty window,
                           * GsxCamera.camera_center; the library exports exactly the functions declared here */

/* Every entry point below is exported; nothing else is (the library is built with -fvisibility=hidden). */
#if defined(__GNUC__)
#define GSX_API __attribute__((visibility("default")))
#else
#define GSX_API
#endif

typedef enum GsxStatus {
    GSX_OK = 0,
    GSX_ERR_INVALID_ARGUMENT = -1,
    GSX_ERR_WORKSPACE_TOO_SMALL = -2, /* stats->n_instances holds the count that is needed */
    GSX_ERR_HIP = -3,                 /* a HIP runtime call or kernel launch failed        */
    GSX_ERR_UNSUPPORTED = -4
} GsxStatus;

/* Compositing semantics. */
typedef enum GsxSemantics {
    /* splat/gaussian_scene.py:146-238: sigmoid applied twice, no alpha clamp, stop when
     * T(1-alpha) < 1e-6 before accumulating, every binned Gaussian evaluated at every pixel of
     * the tile, last tile row/column never rendered, pixel centres at integers. */
    GSX_SEM_REF_CPU = 0,
    /* splat/c/render.cu:21-87: single sigmoid, alpha clamped to 0.99, stop at 0.001, per-pixel
     * inclusive bbox cull, int-truncated means, all tiles rendered. */
    GSX_SEM_REF_CUDA = 1,
    /* Build extension (not in the reference -- parity unpinned): the forward
     * pass of the published 3D Gaussian Splatting rasteriser (Kerbl et al. 2023).  Stage 1: cull
     * z_view <= 0.2, quaternion normalised once, focal = extent / (2 tan(fov/2)), pixel =
     * ((ndc + 1) extent - 1) / 2, 0.3 added to the diagonal of the 2D covariance, symmetric conic,
     * Gaussians with det == 0 or an empty tile rectangle dropped, single sigmoid.  Tiles: every tile
     * whose index lies in [(int)((p - r) / T), (int)((p + r + T - 1) / T)) clamped to the grid, all
     * tiles of the frame (partial edge tiles included).  Per pixel: skip when the exponent is > 0,
     * alpha = min(0.99, opacity * exp(exponent)), skip when alpha < 1/255, stop (before
     * accumulating) when T (1 - alpha) < 1e-4, out = C + T_final * background.  Whole-path entry
     * point only (gsx_render_forward). */
    GSX_SEM_STD_3DGS = 2
} GsxSemantics;

/* Memory layout of the output frame. */
typedef enum GsxLayout {
    GSX_LAYOUT_WH3 = 0, /* out[x][y][c], what render_image returns (gaussian_scene.py:206) */
    GSX_LAYOUT_HW3 = 1  /* out[y][x][c], what render_image_cuda returns (render.cu:116)     */
} GsxLayout;

/*
 * Already-computed float32 camera constants, i.e. the attributes of the reference's
 * GaussianImage that preprocess() reads (splat/image.py:28-66).  Matrices are row-major and in
 * the reference's row-vector convention (p_row @ M).
 */
typedef struct GsxCamera {
    float world2view[16]; /* splat/image.py:51-53  */
    float full_proj[16];  /* splat/image.py:61-65  */
    float tan_fovx;       /* splat/image.py:42     */
    float tan_fovy;       /* splat/image.py:43     */
    float fx;             /* splat/image.py:28     */
    float fy;             /* splat/image.py:29     */
    int32_t width;        /* splat/image.py:38     */
    int32_t height;       /* splat/image.py:37     */
    float camera_center[3]; /* splat/image.py:66 (world2view.inverse()[3,:3]); read only when GsxParams.sh is set */
} GsxCamera;

/*
 * Options.  gsx_default_params() fills the reference's behaviour; a NULL params pointer means
 * the defaults.  The tile window selects which tiles this call renders (multi-GPU strips):
 * tiles [tile_x0, tile_x1) x [tile_y0, tile_y1); tile_x1 / tile_y1 < 0 (the default, -1) means "to the
 * end", tile_x1 == tile_x0 (or y) is an empty window: nothing is rendered, `out` is zeroed.
 * `out` always addresses a buffer of out_w x out_h pixels whose pixel (0,0) is frame pixel
 * (out_x0, out_y0); out_w / out_h <= 0 means the whole frame.
 */
typedef struct GsxParams {
    int32_t semantics; /* GsxSemantics, default GSX_SEM_REF_CPU */
    int32_t layout;    /* GsxLayout, default GSX_LAYOUT_WH3     */
    int32_t tile_x0, tile_x1, tile_y0, tile_y1;
    int32_t out_x0, out_y0, out_w, out_h;
    int32_t flags; /* GSX_FLAG_* */
    float background[3]; /* GSX_SEM_STD_3DGS only: colour behind the last Gaussian (default 0) */
    /* gsx_render_forward only.  NULL (default): the camera constants are the `camera` argument, read at
     * call time.  Otherwise a GsxCamera in DEVICE memory that the projection kernel reads when it RUNS
     * -- the call (and a hipGraph that recorded it) then follows whatever the buffer holds at that
     * moment, e.g. a camera that moves between replays of a captured frame.  `camera` must still be
     * given: its width / height size the frame on the host and must equal the buffer's. */
    const GsxCamera *camera_device;
    /* Optional DEVICE array of one uint32 per tile of the window (window-local id = (tx - tile_x0) *
     * window_height_in_tiles + (ty - tile_y0)): the length of every tile's Gaussian list, written by the
     * frame (all zero when the scene is empty; an empty window has no entries).  What a multi-GPU caller balances
     * its strips with (strips.balanced_plan).  NULL: not reported. */
    uint32_t *tile_counts;
    /* gsx_render_forward only, build extension (the reference has no spherical harmonics).  NULL (default): the
     * `colors` argument is (n,3) RGB.  Otherwise DEVICE coefficients (n, (sh_degree+1)^2, 3), sh_degree in 0..3,
     * in the published 3DGS convention (see gsx_sh_to_rgb); the view-dependent colour is evaluated inside the
     * projection kernel with GsxCamera.camera_center (of `camera`, or of camera_device when that is set), the
     * `colors` argument is ignored and may be NULL. */
    const float *sh;
    int32_t sh_degree;
    /* sizeof(GsxParams) as the CALLER compiled it; gsx_default_params() -- a macro that passes that sizeof -- fills it
     * in.  The fields below it were appended in ABI 300: a struct_size that ends before one of them makes the library
     * ignore that field (a client built against an older header hands over a shorter struct -- whatever lies behind it
     * is neither written by gsx_default_params nor read by any call).  0 = not stated: the struct is taken to be the
     * ABI-300 one, which ends behind `hints` (its callers zeroed this word).  Callers should also check
     * gsx_version() == GSX_VERSION once: the version is bumped whenever a struct or a signature changes. */
    int32_t struct_size;
    /* gsx_render_forward only.  How many Gaussians are expected to reach a tile of the window
     * (GsxFrameStats.n_kept of an earlier frame of this view and window); 0 (default) = unknown, assume all n.
     * A hint, never a bound: it only selects the depth-sort route (the sample-partitioned routes sort what is
     * KEPT inside LDS buckets, so a rank that owns 1/8 of a 5M-Gaussian frame takes the fast route although
     * n is large); a wrong value costs time, not correctness. */
    int64_t kept_hint;
    /* gsx_render_forward only.  NULL (default) or a DEVICE buffer of gsx_hints_bytes() bytes that the caller keeps
     * for ONE view (camera, window, tile size) from frame to frame, zero-filled before its first use.  Two things a
     * frame computes for its own use are correct whatever their values -- the splitters of the depth sort and the
     * order in which tiles are handed to the SIMDs -- so with GSX_FLAG_HINTS_VALID a frame takes both from what the
     * PREVIOUS frame of this view left in the buffer instead of computing them on its own critical path (two
     * dependent kernels, ~20 us of a 0.42 ms frame), and every frame given the buffer leaves fresh ones for the next
     * (computed by spare workgroups of launches that run anyway).  The buffer also holds what every tile COST in the
     * previous frame, which decides which tiles are composited by four waves instead of one (the same pixels either
     * way).  Stale hints (the camera moved) cost time -- unevenly filled sort buckets, an unbalanced hand-out --
     * never a pixel: the frame is the same bit for bit (tested).  Frames in flight on different streams need a
     * buffer each.  The buffer must be 256-byte aligned (GSX_ERR_INVALID_ARGUMENT otherwise). */
    void *hints;
    /* gsx_render_forward only (ABI 302).  Compositing in PARTS, for a caller that wants to start moving a finished part
     * of the window -- a multi-GPU rank sending its strip to the rank that assembles the frame -- while the rest is still
     * being composited: projection, depth order and binning run ONCE for the window, then the compositing launch is
     * issued n_substrips times, part k covering the tiles whose coordinate along `substrip_axis` (0: tile column x, 1:
     * tile row y) lies in [substrip_bounds[k], substrip_bounds[k + 1]), and after the launch of part k the library
     * records substrip_events[k] (a hipEvent_t the caller created) on `stream`.  The pixels are the same bit for bit
     * as those of the one-launch frame.  substrip_bounds: HOST array of n_substrips + 1 absolute tile coordinates,
     * ascending, [0] = the window's first and [n_substrips] = its last + 1 tile along that axis; substrip_events: HOST
     * array of n_substrips events.  n_substrips 0 or 1 (default): one launch, nothing recorded.  At most 16 parts.
     * Not while `stream` is being captured into a hipGraph (GSX_ERR_UNSUPPORTED): the events are recorded on the stream.
     * Rule sets / tile sizes without a partial launch composite in one launch and record every event behind it. */
    int32_t n_substrips;
    int32_t substrip_axis;
    const int32_t *substrip_bounds;
    void *const *substrip_events;
    /* sizeof(GsxFrameStats) as the CALLER compiled it (ABI 305); gsx_default_params() fills it in.  The render calls write
     * `stats_host` only that far: 64 bytes (n_visible .. n_kept, the struct of ABI 300) or 72 (+ n_redo).  A caller whose
     * GsxParams ends before this field, or who passes params == NULL, is taken to own the 64-byte struct and gets no n_redo
     * (GsxFrameStats grew once, in ABI 303, with nothing to tell the two apart: INTEGRATION.md's stub was overrun by 8 bytes).
     * Any other value is GSX_ERR_INVALID_ARGUMENT.  Every later field of GsxFrameStats will be reported the same way. */
    int32_t stats_size;
    int32_t reserved1; /* 0 */
    /* gsx_render_forward / gsx_preprocess (ABI 305).  NULL (default): Gaussian i of the input arrays IS Gaussian i.  Otherwise
     * a DEVICE array of n int32, a permutation of 0 .. n-1: the caller has REORDERED its five parameter arrays (and `sh`) -- e.g.
     * along a space-filling curve, so that the Gaussians of one part of the frame lie together in memory and a rank that
     * renders a strip reads AND WRITES whole cache lines of survivors (Gaussians.spatially_ordered() of the Python surface)
     * -- and row i of them holds the Gaussian whose ORIGINAL index is original_index[i].  The frame is then the one the
     * original arrays give, bit for bit: the depth keys are filed under the original index and the depth sort enumerates
     * them in that order, so equal depths still composite in original-index order; `order` and every reported index is the
     * original one.  gsx_render_forward also needs the inverse, row_of_index (below): records and rectangles stay in ROW
     * order -- written and, tile by tile, read back as neighbours -- and the sort's first pass turns an original index into
     * the row it names. */
    const int32_t *original_index;
    /* gsx_render_forward, with original_index (ABI 305).  NULL (default) or a DEVICE array of 8 floats per block of
     * GSX_BOUNDS_ROWS consecutive ROWS of the (reordered) arrays -- (min x, min y, min z, largest |scale|, max x, max y, max z,
     * 0) over the block's means and scales; ceil(n / GSX_BOUNDS_ROWS) blocks.  A call that renders a PART of the frame then
     * drops a whole block after reading these 32 bytes when the projected box, grown by the largest footprint radius any of
     * its Gaussians can have, misses the tile window and lies in front of the cull plane -- instead of reading 24 bytes of
     * every Gaussian to find the same thing out row by row.  Conservative: a block is only dropped when each of its rows
     * would be; the frame is the same bit for bit.  The bounds describe the arrays AS THEY ARE: whoever moves a mean or
     * grows a scale recomputes them (the Python surface does, from torch's in-place version counters:
     * Gaussians.current_block_bounds()). */
    const float *block_bounds;
    /* gsx_render_forward, with original_index: DEVICE array of n int32, the inverse permutation -- row_of_index[original_index[i]]
     * == i.  Required there (GSX_ERR_INVALID_ARGUMENT without it); gsx_preprocess does not read it. */
    const int32_t *row_of_index;
} GsxParams;
#define GSX_BOUNDS_ROWS 256

/* Record per-stage GPU times with HIP events on `stream` into GsxFrameStats.stage_ms (the call
 * then waits for the frame to finish).  Off by default: timing is measurement, not product. */
#define GSX_FLAG_TIMING 1

/* Enqueue the frame without waiting for the device at all.  Normally a render call synchronises
 * the stream once, after its last launch, to fill stats_host and to detect a pair count beyond
 * the workspace capacity.  With this flag it returns as soon as the launches are queued:
 * stats_host must then be PINNED host memory that stays valid until the stream has passed this
 * frame; n_visible / n_instances arrive by an asynchronous copy (stats_host->reserved holds the
 * pair capacity the frame was enqueued with, > 0); read them after synchronising the stream.  If
 * n_instances turns out larger than that capacity, pairs were dropped and the frame must be
 * rendered again with a larger workspace. */
#define GSX_FLAG_NO_SYNC 2

/* Composite with the any-tile-size kernels (one pixel per lane) even when tile == 16, where the
 * specialised 4-pixels-per-lane kernels would run.  Same arithmetic, same pixels bit for bit; exists
 * so that tests can hold the two kernel families against each other. */
#define GSX_FLAG_GENERIC_KERNELS 4

/* GSX_SEM_STD_3DGS only.  By default a Gaussian is binned into the tiles met by the bounding box of
 * the ellipse on which its alpha reaches 1/255 (with a 1 % safety margin on alpha), intersected with
 * the published rectangle (the square of the 3-sigma radius): a pixel outside that ellipse is skipped
 * by the alpha < 1/255 rule anyway, so the frame is the same bit for bit while the tile lists get
 * shorter (24 % fewer pairs on the benchmark scene; a Gaussian whose opacity is below 1/255 is in
 * no tile at all).  This flag bins with the published rectangles instead, e.g. to compare
 * GsxFrameStats.n_instances with another implementation of the published algorithm. */
#define GSX_FLAG_PUBLISHED_RECTS 8

/* GSX_SEM_REF_CPU, tile 16.  By default a tile whose Gaussian list is more than 4x the frame's average (and
 * more than 1024 entries) long is composited by four waves -- a quarter of its pixels each, one pixel per
 * lane -- instead of one, so that a few very long lists (trained scenes are heavy-tailed) do not outlast
 * the rest of the frame.  Same arithmetic, same pixels bit for bit; this flag keeps every tile on one wave,
 * for tests that hold the two paths against each other. */
#define GSX_FLAG_NO_LONG_TILE_SPLIT 16

/* Tile 16, GSX_SEM_REF_CPU / GSX_SEM_STD_3DGS.  All the tile workgroups of a 1080p frame are resident at once, so
 * a SIMD is busy for as long as the lists of its own tiles take; frames of >= 300 000 Gaussians therefore run one
 * more small kernel that ranks the tiles by list length (windows of more than 2048 tiles), and the compositing launch hands them out so that every
 * SIMD gets its share of every length class.  Which workgroup composites which tile does
 * not touch a pixel: the frame is the same bit for bit.  GSX_FLAG_TILE_SCHEDULE asks for the schedule whatever
 * the size of the scene, GSX_FLAG_NO_TILE_SCHEDULE never builds it (tests hold the two against each other). */
#define GSX_FLAG_TILE_SCHEDULE 32
#define GSX_FLAG_NO_TILE_SCHEDULE 64

/* GsxParams.hints holds what an earlier frame of the same view (same buffer, same n, same window and tile size) left
 * there: use it.  Without the flag a frame given a hints buffer only fills it. */
#define GSX_FLAG_HINTS_VALID 128

/* gsx_render_forward / gsx_preprocess, GSX_SEM_REF_CPU and GSX_SEM_REF_CUDA: how many Gaussians the reference has
 * VISIBLE when that is at most three.  Its matrix products over the visible Gaussians -- [p,1] @ world2view
 * (splat/gaussian_scene.py:79-85, splat/utils.py:333) and ... @ W.T (splat/utils.py:354) -- are single BLAS calls, and
 * the BLAS it runs on (MKL under torch) sums an output's products as a sequential FMA chain from four rows up, as
 * (k0 + k2) + (k1 + k3) unfused on two or three rows and in a third order on one (oracle/probe_torch_order.py).  A
 * call does not know N_vis while it projects: it assumes all n Gaussians are visible (n <= 3 selects the few-row
 * orders by itself).  A frame that reports another class (GsxFrameStats.n_visible = 1, or 2..3, out of more) differs
 * from the reference in the last bit of up to three depths and 2D covariances; a caller that wants the reference's
 * bits there too issues the call again with the flag that names the class -- the Python surface does. */
#define GSX_FLAG_SMALL_BATCH 256  /* two or three Gaussians are visible */
#define GSX_FLAG_ONE_VISIBLE 512  /* exactly one is */

/* gsx_render_forward / gsx_render_preprocessed, GSX_SEM_REF_CPU at tile size 16.  The compositing launch evaluates
 * ill-conditioned footprints (axis ratios from ~20:1, on the tiles along their ridge) in the reference's own float32
 * operation order; how many tiles and long-tile quarters held one is GsxFrameStats.n_redo.  With
 * this flag the call runs the instance of that launch that CANNOT evaluate them -- half the registers, twice the waves
 * per SIMD, ~6 % faster on a 4K frame of 5M Gaussians, no faster at 1080p -- for a caller that knows from an earlier frame
 * of the same view that n_redo was 0.  The frame's own n_redo says whether that held: if it is > 0, that many tiles /
 * quarters were NOT composited (their pixels are unspecified) and the frame must be rendered again without the flag.
 * A call that could not report n_redo -- stats_host NULL, or GsxParams.stats_size < 72 -- is refused with the flag set
 * (GSX_ERR_INVALID_ARGUMENT): the caller MUST be able to read it. */
#define GSX_FLAG_PLAIN_FOOTPRINTS 1024

/* GSX_SEM_STD_3DGS only: the anti-aliased variant of the published rule set (Mip-Splatting's 2D filter, the published
 * rasteriser's `antialiasing` switch, gsplat's rasterize_mode="antialiased").  Stage 1 still adds 0.3 to the diagonal of
 * the 2D covariance, and now multiplies the opacity by
 *     rho = sqrt(max(0.000025, det0 / det1)),   det0 = ca cd - cb cb before the dilation, det1 after it,
 * so that the widened Gaussian carries the energy of the original: alpha = min(0.99, sigmoid(logit) rho exp(exponent)),
 * and the 1/255 skip, the 0.99 clamp and the stop rule all see that product.  Conic, radius and tile rectangles are the
 * flag-clear call's (the rectangles are sized by sigmoid(logit): the same pairs are listed, more of them are skipped).
 * Where det0 / det1 <= 0.000025 -- a float32 det0 <= 0 included -- rho is the constant 0.005 and carries no gradient.
 * Honoured by gsx_render_forward, gsx_render_backward_std (dL/dlogit = (sum u)(1 - sigmoid(logit)), and dL/drho reaches
 * scales, quaternions and points through the 2D covariance) and gsx_render_contribution.  GSX_ERR_INVALID_ARGUMENT under
 * the other two semantics and from every entry that does not take GSX_SEM_STD_3DGS.  With the flag clear every output
 * of every entry keeps its bits. */
#define GSX_FLAG_ANTIALIASED 2048

/* Indices into GsxFrameStats.stage_ms (milliseconds). */
enum {
    GSX_STAGE_PROJECT = 0,    /* projection, depth keys, record packing         */
    GSX_STAGE_DEPTH_SORT = 1, /* stable sort of the depth keys (drops Gaussians that reach no tile) */
    GSX_STAGE_SCAN = 2,       /* tile-count sums + (tile, Gaussian) pair emission */
    GSX_STAGE_BIN = 3,        /* tile sort, tile ranges (+ the compositing schedule) */
    GSX_STAGE_BLEND = 4,      /* the compositing kernel alone                   */
    GSX_STAGE_TOTAL = 5
};

/* Host-side counts of one frame (N_vis and D). */
typedef struct GsxFrameStats {
    int64_t n_visible;   /* Gaussians that pass the z_view >= 0.2 cull         */
    int64_t n_instances; /* (Gaussian, tile) pairs binned inside the tile window */
    int64_t n_tiles;     /* tiles inside the window                             */
    int64_t reserved;
    float stage_ms[6];   /* filled only with GSX_FLAG_TIMING                     */
    int64_t n_kept;      /* Gaussians that reach a tile of the window (what the depth sort keeps): GsxParams.kept_hint
                          * of the next frame of this view                       */
    int64_t n_redo;      /* tiles (and long-tile quarters) that held an ill-conditioned footprint; see
                          * GSX_FLAG_PLAIN_FOOTPRINTS (ABI 303: the struct has 72 bytes).  Written only when
                          * GsxParams.stats_size >= 72 says the caller's struct has it */
} GsxFrameStats;
#define GSX_FRAME_STATS_BYTES_ABI300 64 /* n_visible .. n_kept: what a call writes when it is not told the struct's size */

GSX_API int gsx_version(void);
GSX_API const char *gsx_last_error(void);
/* Fills the first `struct_size` bytes of *params -- sizeof(GsxParams) as the caller compiled it -- with the reference's
 * behaviour and states that size in GsxParams.struct_size.  Nothing behind those bytes is touched. */
GSX_API void gsx_default_params_sized(GsxParams *params, size_t struct_size);
/* What callers write: the size is this header's.  (The exported FUNCTION of this name exists for binaries built
 * against the ABI 300 / 301 headers, where the struct had 104 bytes: it fills those and states struct_size = 104 -- so
 * the fields appended since (n_substrips .., stats_size) are NOT read from a struct filled through it.  A binary built
 * against the 302 header, the only one that had those fields AND called this function, must be rebuilt: its
 * substrip_events would never be recorded.  Language bindings call gsx_default_params_sized.) */
GSX_API void gsx_default_params(GsxParams *params);
#define gsx_default_params(params) gsx_default_params_sized((params), sizeof(GsxParams))

/*
 * Bytes of device workspace needed by any entry point below for up to `n` Gaussians, a
 * width x height frame, tile size `tile` and at most `max_instances` (Gaussian, tile) pairs.
 * Returns 0 on invalid arguments.
 */
GSX_API size_t gsx_workspace_bytes(int64_t n, int32_t width, int32_t height, int32_t tile, int64_t max_instances);

/* Bytes of a GsxParams.hints buffer for frames of width x height at tile size `tile` (0 on invalid arguments). */
GSX_API size_t gsx_hints_bytes(int32_t width, int32_t height, int32_t tile);

/*
 * Stage 1.  Replaces GaussianScene.preprocess (splat/gaussian_scene.py:70-144) with
 * Gaussians.get_3d_covariance_matrix (splat/gaussians.py:54-69) and the helpers of
 * splat/utils.py:293-423 fused in.  Inputs are the Gaussians attributes (splat/gaussians.py:19-33):
 * means3d (n,3), scales (n,3) linear, quats (n,4) (w,x,y,z), opacity_logit (n,1), colors (n,3).
 * Outputs are the PreprocessedScene fields (splat/schema.py:13-25), each with room for n rows,
 * depth-sorted (ascending view z, ties by original index); rows >= *n_visible_host are unspecified.
 * order (n) int32: original index of each sorted row (may be NULL).  Synchronises `stream`.
 */
GSX_API int gsx_preprocess(const GsxCamera *camera, const float *means3d, const float *scales, const float *quats,
                   const float *opacity_logit, const float *colors, int64_t n,
                   float *points_xy, float *colors_out, float *covariance_2d, float *depths,
                   float *inverse_covariance_2d, float *radius, float *min_x, float *max_x,
                   float *min_y, float *max_y, float *sigmoid_opacity, int32_t *order,
                   int64_t *n_visible_host, const GsxParams *params, void *workspace,
                   size_t workspace_bytes, void *stream);

/*
 * Stage 2 on stage-1 arrays.  Argument-for-argument mirror of the reference's native entry
 * point `torch::Tensor render_image(int image_height, int image_width, int tile_size, point_means,
 * point_colors, inverse_covariance_2d, min_x, max_x, min_y, max_y, opacity)`
 * (splat/c/render.cu:90-101, declared at splat/gaussian_scene.py:244-257), with the output
 * buffer caller-allocated instead of returned.  Rows must be in compositing (depth) order.
 * `opacity` is PreprocessedScene.sigmoid_opacity (n,1).  Under GSX_SEM_REF_CPU this computes what
 * GaussianScene.render_image (splat/gaussian_scene.py:200-238) computes from the same arrays.
 * out_image is fully written (pixels outside rendered tiles are set to 0).
 */
GSX_API int gsx_render_preprocessed(int32_t image_height, int32_t image_width, int32_t tile_size,
                            const float *point_means, const float *point_colors,
                            const float *inverse_covariance_2d, const float *min_x, const float *max_x,
                            const float *min_y, const float *max_y, const float *opacity, int64_t n,
                            float *out_image, const GsxParams *params, GsxFrameStats *stats_host,
                            void *workspace, size_t workspace_bytes, void *stream);

/*
 * Whole hot path: projection -> depth order -> tile binning -> compositing.  Replaces
 * GaussianScene.render_image (splat/gaussian_scene.py:200-238) and, with GSX_SEM_REF_CUDA /
 * GSX_LAYOUT_HW3, GaussianScene.render_image_cuda (splat/gaussian_scene.py:263-285); with
 * GSX_SEM_STD_3DGS (build extension) it is the forward pass of the published 3DGS rasteriser.
 * stats_host may be NULL.  Synchronises `stream` once, after the last launch, to report the counts
 * and to detect n_instances > capacity (GSX_ERR_WORKSPACE_TOO_SMALL; stats_host->n_instances then
 * holds the count to size the workspace for); with GSX_FLAG_NO_SYNC it does not synchronise at all.
 */
GSX_API int gsx_render_forward(const GsxCamera *camera, const float *means3d, const float *scales, const float *quats,
                       const float *opacity_logit, const float *colors, int64_t n, int32_t tile_size,
                       float *out_image, const GsxParams *params, GsxFrameStats *stats_host,
                       void *workspace, size_t workspace_bytes, void *stream);

/*
 * Backward pass of gsx_render_forward under GSX_SEM_REF_CPU: the gradients the reference's autograd produces for
 * L(frame), with grad_image = dL/dframe (same layout as the frame, GsxParams.layout), with respect to the colours
 * (grad_colors, n x 3) and the opacity logits (grad_opacity_logit, n x 1).  The means, scales and quaternions get none
 * here, as under the reference's autograd, whose Gaussian weight is a Python float (splat/utils.py:357-365): use
 * gsx_render_backward_geometry for those.  `image` is the frame gsx_render_forward
 * produced from the same inputs and params (its pixels enter every gradient).  Projection, depth order and binning are
 * run again (deterministic: the same lists as the forward's); GsxParams.hints is neither read nor written.  Every row
 * of both outputs is written (0 for a Gaussian on no tile list).  Same inputs, same bits: no float atomics.
 * Refused with GSX_ERR_INVALID_ARGUMENT: other semantics, GsxParams.sh (an SH scene passes the colours gsx_sh_to_rgb evaluated
 * and carries grad_colors on to its coefficients with gsx_sh_backward), a tile window, an output window, substrips,
 * GSX_FLAG_NO_SYNC, camera_device.  workspace: gsx_backward_workspace_bytes(n, width, height, tile, pairs) with at
 * least the frame's pair count (GsxFrameStats.n_instances of the forward); fewer: GSX_ERR_WORKSPACE_TOO_SMALL.
 * Synchronises `stream`.
 */
GSX_API int gsx_render_backward(const GsxCamera *camera, const float *means3d, const float *scales, const float *quats,
                        const float *opacity_logit, const float *colors, int64_t n, int32_t tile_size,
                        const float *image, const float *grad_image, float *grad_colors, float *grad_opacity_logit,
                        const GsxParams *params, void *workspace, size_t workspace_bytes, void *stream);

/* Bytes of device workspace gsx_render_backward needs (0 on invalid arguments). */
GSX_API size_t gsx_backward_workspace_bytes(int64_t n, int32_t width, int32_t height, int32_t tile, int64_t max_instances);

/*
 * gsx_render_backward plus the geometry: also dL/dmeans3d (grad_means3d, n x 3), dL/dscales (grad_scales, n x 3, linear
 * scales) and dL/dquats (grad_quats, n x 4, (w,x,y,z); orthogonal to the quaternion up to rounding, since the forward
 * normalises it) -- what the reference's graph gives once its Gaussian weight stays a tensor: through the pixel mean and
 * the inverse 2D covariance of every composited (Gaussian, pixel), the floored determinant (floored: the adjugate alone
 * carries gradient), the EWA projection with its 1.3 tan(fov / 2) clamp, Sigma = (R S)(R S)^T and the quaternion normalised
 * twice.  The tile rectangle, radius, culling and depth order are piecewise constant: no gradient.  All five outputs are
 * written for every row (exact zeros for a Gaussian that is culled or on no tile list); grad_colors and
 * grad_opacity_logit hold the bits gsx_render_backward writes.  Same refusals, same synchronisation, no hints touched,
 * no float atomics: same inputs, same bits.  workspace: gsx_backward_geometry_workspace_bytes.
 */
GSX_API int gsx_render_backward_geometry(const GsxCamera *camera, const float *means3d, const float *scales, const float *quats,
                                 const float *opacity_logit, const float *colors, int64_t n, int32_t tile_size,
                                 const float *image, const float *grad_image, float *grad_colors, float *grad_opacity_logit,
                                 float *grad_means3d, float *grad_scales, float *grad_quats, const GsxParams *params,
                                 void *workspace, size_t workspace_bytes, void *stream);

/* Bytes of device workspace gsx_render_backward_geometry needs (0 on invalid arguments). */
GSX_API size_t gsx_backward_geometry_workspace_bytes(int64_t n, int32_t width, int32_t height, int32_t tile, int64_t max_instances);

/*
 * gsx_render_backward_geometry plus what screen-space density control reads (gsx_density_accumulate_screen): the same
 * arguments with two more outputs behind grad_quats, the same refusals (and grad_means2d NULL), the same synchronisation, the
 * same workspace (gsx_backward_geometry_workspace_bytes), no float atomics: same inputs, same bits.  The five older outputs
 * hold the bits gsx_render_backward_geometry writes.
 *   grad_means2d (n,2), required: dL/d(NDC mean), the published trainer's viewspace_points.grad[:, :2]:
 *       (dL/dmean_x (width - 1) / 2,  dL/dmean_y (height - 1) / 2),   dL/dmean = -1/2 (Q + Q^T) sum u d
 *     over every composited (Gaussian, pixel), with d = mean - pixel in pixels and u = dL/dpower -- the very values the chain
 *     to dL/dmeans3d starts from.  In float32, from the Gaussian's moment sums S1 = sum u d0, S2 = sum u d1 and the conic Q as
 *     the frame's record stores it:
 *       gmx = -0.5f * (2.0f * q00 * S1 + (q01 + q10) * S2)        gmy = -0.5f * ((q01 + q10) * S1 + 2.0f * q11 * S2)
 *       grad_means2d = (gmx * sx, gmy * sy),   sx = ((float)width - 1.0f) * 0.5f,   sy = ((float)height - 1.0f) * 0.5f
 *     every operation rounded on its own, the products and sums left to right as written.  It is the rasteriser's share
 *     only: for an SH scene the view direction's share of dL/dmeans3d (gsx_sh_backward) is not in it, as published.
 *   screen_radius (n), may be NULL: for a Gaussian on at least one tile list of the frame the forward's radius in pixels,
 *     ceilf(3 sqrtf(lam)) -- the bits gsx_preprocess reports in `radius`, in the row class the call runs with
 *     (GSX_FLAG_ONE_VISIBLE / GSX_FLAG_SMALL_BATCH).
 * Both are written for every row: exact +0 for a Gaussian that is culled or on no tile list, so screen_radius > 0 says
 * "this frame listed the Gaussian", whatever its gradient.
 */
GSX_API int gsx_render_backward_screen(const GsxCamera *camera, const float *means3d, const float *scales, const float *quats,
                               const float *opacity_logit, const float *colors, int64_t n, int32_t tile_size,
                               const float *image, const float *grad_image, float *grad_colors, float *grad_opacity_logit,
                               float *grad_means3d, float *grad_scales, float *grad_quats, float *grad_means2d,
                               float *screen_radius /* may be NULL */, const GsxParams *params, void *workspace,
                               size_t workspace_bytes, void *stream);

/*
 * gsx_render_backward_screen plus the ABSOLUTE screen statistic (AbsGS's answer to "gradient collision", gsplat's absgrad): the
 * same arguments with one more output behind screen_radius, the same refusals (and grad_means2d, screen_radius or
 * grad_means2d_abs NULL: all three are required here), the same synchronisation, the same workspace
 * (gsx_backward_geometry_workspace_bytes), no float atomics: same inputs, same bits.  The seven older outputs hold the bits
 * gsx_render_backward_screen writes.
 *   grad_means2d_abs (n,2): grad_means2d is a signed sum over the pixels a Gaussian touches, and over fine detail the terms
 *     cancel.  This is the sum of their absolute values, per component.  For every composited (Gaussian, pixel), with u and
 *     d = mean - pixel as above, u0 = u * d0, u1 = u * d1 (the products S1 and S2 add up) and the conic as stored:
 *       tx = fmaf(2.0f * q00, u0, (q01 + q10) * u1)              ty = fmaf(q01 + q10, u0, (2.0f * q11) * u1)
 *       Tx = sum |tx|,  Ty = sum |ty|      over the pixels of every tile that composites the Gaussian, under the stop rule
 *       grad_means2d_abs = ((0.5f * Tx) * |sx|, (0.5f * Ty) * |sy|)
 *     so that the same sums WITHOUT the absolute value are grad_means2d up to rounding, and grad_means2d_abs >= |grad_means2d|
 *     componentwise up to rounding.  The sums run in a fixed order: per tile over the lane's pixels, then a fixed butterfly
 *     over the wave, the chunks of a tile of more than 256 pixels in rising order; per Gaussian over its tiles lane-strided
 *     in emission order, then the same butterfly.  Written for every row: exact +0 for a Gaussian that is culled or on no
 *     tile list.  gsx_density_accumulate_screen takes it in place of grad_means2d; the published threshold of 2e-4
 *     belongs to the signed statistic, not to this one.
 */
GSX_API int gsx_render_backward_screen_abs(const GsxCamera *camera, const float *means3d, const float *scales, const float *quats,
                                   const float *opacity_logit, const float *colors, int64_t n, int32_t tile_size,
                                   const float *image, const float *grad_image, float *grad_colors, float *grad_opacity_logit,
                                   float *grad_means3d, float *grad_scales, float *grad_quats, float *grad_means2d,
                                   float *screen_radius, float *grad_means2d_abs, const GsxParams *params, void *workspace,
                                   size_t workspace_bytes, void *stream);

/*
 * gsx_render_backward_screen plus the camera: the same arguments with two more device outputs behind screen_radius, the same
 * refusals (grad_world2view or grad_full_proj NULL besides; grad_means2d and screen_radius may BOTH be NULL here), the same
 * synchronisation, no hints touched, no float atomics: same inputs, same bits.  The older outputs hold the bits
 * gsx_render_backward_screen writes.  workspace: gsx_backward_camera_workspace_bytes.
 *   grad_world2view[16], grad_full_proj[16]: dL/d(entry) of GsxCamera.world2view and GsxCamera.full_proj, row-major in
 *     the camera's own row-vector convention, the two matrices taken as INDEPENDENT inputs (a caller whose full_proj is
 *     world2view @ P adds grad_full_proj @ P^T) and everything else of the camera (fx, fy, tan_fov*, camera_center) as
 *     constant.  Per Gaussian on a tile list, with p the point, g_t the gradient of the view-space point t = [p,1] world2view,
 *     dT the gradient of T = J W (W[i][j] = world2view[j][i], J the 2x3 EWA Jacobian) and gh the gradient of the homogeneous
 *     point h = [p,1] full_proj (columns 0, 1, 3):
 *       grad_world2view[k][c] += p_k g_t[c] + (J[0][c] dT[0][k] + J[1][c] dT[1][k])   (k, c < 3)
 *       grad_world2view[3][c] += g_t[c]
 *       grad_full_proj[k][c] += p_k gh_c,   grad_full_proj[3][c] += gh_c               (c in {0, 1, 3})
 *     Column 3 of grad_world2view and column 2 of grad_full_proj are exact +0: nothing the frame computes reads them.  The
 *     branch decisions (floored determinant, active clamp, culling, tile lists, stop) are piecewise constant.  A frame that
 *     lists nothing writes 32 exact +0.  The sum over Gaussians runs in a fixed order: per 256 depth ranks the wave
 *     butterflies and the four waves in order, then the blocks in eight interleaved stripes, each in rising order.
 */
GSX_API int gsx_render_backward_camera(const GsxCamera *camera, const float *means3d, const float *scales, const float *quats,
                               const float *opacity_logit, const float *colors, int64_t n, int32_t tile_size,
                               const float *image, const float *grad_image, float *grad_colors, float *grad_opacity_logit,
                               float *grad_means3d, float *grad_scales, float *grad_quats, float *grad_means2d /* may be NULL */,
                               float *screen_radius /* may be NULL */, float *grad_world2view, float *grad_full_proj,
                               const GsxParams *params, void *workspace, size_t workspace_bytes, void *stream);

/* Bytes of device workspace gsx_render_backward_camera needs (0 on invalid arguments). */
GSX_API size_t gsx_backward_camera_workspace_bytes(int64_t n, int32_t width, int32_t height, int32_t tile, int64_t max_instances);

/*
 * Expected depth and coverage of the GSX_SEM_REF_CPU frame: depth_out holds, per pixel, the two floats
 *   D = sum_k T_k alpha_k z_k        A = sum_k T_k alpha_k
 * over the pixel's tile list in list order, with the frame's two leading axes (GsxParams.layout) and 2 floats where the
 * frame has 3.  alpha_k is the reference's alpha in the reference's operation order, T_1 = 1, the pixel stops before the
 * first record with T_k (1 - alpha_k) < 1e-6 (a NaN stops it too) and EVERY listed record is walked: the gradient
 * entries' walk, without gsx_render_forward's skip of records below 2^-26.  z_k is the view-space depth the depth order is
 * built on -- the reference's points_view[:, 2], gsx_preprocess' `depths` -- in the row class the call runs with
 * (GSX_FLAG_ONE_VISIBLE / GSX_FLAG_SMALL_BATCH).  D is not divided by A.  Every pixel is written: exact +0 where the frame
 * has zeros (the last row and column of tiles, which REF_CPU does not render, and a frame that lists nothing).
 * Projection, depth order and binning run again, as for gsx_render_backward: GsxParams.hints is neither read nor written.
 * `colors` is read by that chain only (no depth depends on it).  The refusals and the synchronisation are
 * gsx_render_backward's.  workspace: gsx_depth_workspace_bytes(n, width, height, tile, pairs) with at least the frame's
 * pair count.
 */
GSX_API int gsx_render_depth(const GsxCamera *camera, const float *means3d, const float *scales, const float *quats,
                     const float *opacity_logit, const float *colors, int64_t n, int32_t tile_size, float *depth_out,
                     const GsxParams *params, void *workspace, size_t workspace_bytes, void *stream);

/* Bytes of device workspace gsx_render_depth needs (0 on invalid arguments). */
GSX_API size_t gsx_depth_workspace_bytes(int64_t n, int32_t width, int32_t height, int32_t tile, int64_t max_instances);

/*
 * gsx_render_backward_screen for L(frame, depth image): the same arguments with the image gsx_render_depth wrote (`depth`)
 * and dL/d(that image) (`grad_depth`, same layout) behind screen_radius; grad_means2d and screen_radius may BOTH be NULL.
 * With gD = dL/dD and gA = dL/dA of a pixel, D_k and A_k its running sums including record k:
 *   dL/dz_k      = sum over pixels T_k alpha_k gD, summed per Gaussian into Sz;  grad_means3d += Sz world2view[0:3][2]
 *   dL/dalpha_k += T_k (z_k gD + gA) - ((D - D_k) gD + (A - A_k) gA) / (1 - alpha_k)
 * added to the frame's dL/dalpha_k before anything is formed from it: grad_opacity_logit, grad_means3d, grad_scales,
 * grad_quats, grad_means2d take depth's share through the same sums and the same chain (screen_radius is the forward's
 * value as before; grad_colors gets nothing from depth).  The tile rectangle, culling and depth order are piecewise
 * constant; the camera is a constant.  With grad_depth all +0 every output holds the bits gsx_render_backward_screen
 * writes.  Same refusals (depth or grad_depth NULL besides), same synchronisation, no hints touched, no float atomics:
 * same inputs, same bits.  workspace: gsx_backward_depth_workspace_bytes.
 */
GSX_API int gsx_render_backward_depth(const GsxCamera *camera, const float *means3d, const float *scales, const float *quats,
                              const float *opacity_logit, const float *colors, int64_t n, int32_t tile_size,
                              const float *image, const float *grad_image, float *grad_colors, float *grad_opacity_logit,
                              float *grad_means3d, float *grad_scales, float *grad_quats, float *grad_means2d /* may be NULL */,
                              float *screen_radius /* may be NULL */, const float *depth, const float *grad_depth,
                              const GsxParams *params, void *workspace, size_t workspace_bytes, void *stream);

/* Bytes of device workspace gsx_render_backward_depth needs (0 on invalid arguments). */
GSX_API size_t gsx_backward_depth_workspace_bytes(int64_t n, int32_t width, int32_t height, int32_t tile, int64_t max_instances);

/*
 * BUILD EXTENSION -- gradients of the GSX_SEM_STD_3DGS frame (the published rule set: 0.3 dilation, alpha clamped at 0.99,
 * the 1/255 skip, stop before the pair with T (1 - alpha) < 1e-4, background behind the last Gaussian).
 * params->semantics must be GSX_SEM_STD_3DGS; params->background, GSX_FLAG_PUBLISHED_RECTS and GSX_FLAG_ANTIALIASED (the
 * frame's opacity is sigmoid(logit) rho: dL/dlogit and the geometry gradients follow it, see the flag) are honoured as in
 * gsx_render_forward, so the tile lists are that frame's.  image: the frame gsx_render_forward wrote for these inputs and
 * params (whole frame, params->layout); grad_image: dL/dimage, same layout.  Per pixel the forward's walk is repeated with
 * the forward's operations and its three decisions; with g = dL/dpixel and F the pixel (T_fin background included):
 *     dL/dc_k = T_k alpha_k g        dL/dalpha_k = T_k (c_k . g) - (F - C_k) . g / (1 - alpha_k)
 * and u_k = dL/dalpha_k alpha_k where the clamp is inactive (opacity exp(power) < 0.99f), 0 where it is active: a clamped
 * pair reaches its colour only.  dL/dlogit = (sum u)(1 - opacity), opacity = sigmoid(logit) once.  dL/dbackground is not
 * computed.
 * grad_means3d, grad_scales, grad_quats: all three or all NULL (NULL: the colour-only kernel runs; grad_colors and
 * grad_opacity_logit are the same bits either way).  With them the moments of u reach the inputs through the rule set's own
 * stage 1: quaternion normalised once, the dilation a constant, conic = adj / det without a floor, p_w = 1 / (w + 1e-7),
 * pixel = ((ndc + 1) dim - 1) / 2, the 1.3 tan(fov / 2) clamp decided on float32 values formed in stage 1's order.
 * grad_means2d (n,2) and screen_radius (n): both or both NULL, and only with the geometry three: dL/d(NDC mean) =
 * dL/d(pixel mean) * (width / 2, height / 2) and the published radius ceil(3 sqrt(lambda_max)) in pixels, as
 * gsx_density_accumulate_screen reads them.
 * Every output row is written: exact zeros for a Gaussian that is culled or on no tile list.  Projection, depth order and
 * binning are run again; GsxParams.hints is not touched; synchronises `stream`.  Refused like gsx_render_backward: tile
 * window, output window, substrips, GSX_FLAG_NO_SYNC, camera_device, params->sh -- and any semantics but
 * GSX_SEM_STD_3DGS.  Bad arguments are refused by name before any HIP call.  No float atomics: same inputs, same bits.
 * workspace: gsx_backward_std_workspace_bytes.
 */
GSX_API int gsx_render_backward_std(const GsxCamera *camera, const float *means3d, const float *scales, const float *quats,
                                    const float *opacity_logit, const float *colors, int64_t n, int32_t tile_size,
                                    const float *image, const float *grad_image, float *grad_colors, float *grad_opacity_logit,
                                    float *grad_means3d, float *grad_scales, float *grad_quats, float *grad_means2d,
                                    float *screen_radius, const GsxParams *params, void *workspace, size_t workspace_bytes,
                                    void *stream);

/* Bytes of device workspace gsx_render_backward_std needs, with or without the geometry outputs (0 on invalid arguments). */
GSX_API size_t gsx_backward_std_workspace_bytes(int64_t n, int32_t width, int32_t height, int32_t tile, int64_t max_instances);

/*
 * Build extension: what every Gaussian contributes to one frame.  For a (record k, pixel) pair that the walk composites,
 * w = T_k alpha_k is the record's blend weight in that pixel -- the factor its colour enters the pixel with.  Per row:
 *   weight_max (n)  the largest w over the frame's pixels        (RadSplat's prune score, maximised over the views)
 *   weight_sum (n)  the sum of w over the frame's pixels         (the score LightGaussian and Mini-Splatting rank on)
 *   pixels     (n)  the number of pixels that composited the row
 *   views      (n)  1 where the frame listed the row on a tile; may be NULL
 * Projection, depth order, binning and the emission prefix run again exactly as for gsx_render_backward /
 * gsx_render_backward_std: hints are neither read nor written, the row classes (GSX_FLAG_ONE_VISIBLE / _SMALL_BATCH) and
 * the one synchronisation are theirs, GSX_FLAG_PUBLISHED_RECTS and GSX_FLAG_ANTIALIASED (the weights of the anti-aliased
 * frame) are honoured under GSX_SEM_STD_3DGS (the background changes nothing here).  params->semantics is GSX_SEM_REF_CPU (NULL params: that) or GSX_SEM_STD_3DGS; GSX_SEM_REF_CUDA is
 * refused, and so is everything the gradient entries refuse: tile window, output window, substrips, GSX_FLAG_NO_SYNC,
 * camera_device, params->sh.
 * The walk is the GRADIENT entries' walk, not the forward's.  GSX_SEM_REF_CPU: the reference's alpha on every listed record
 * (no 2^-26 skip), the pixel stopped before the record that would take its transmittance below 1e-6; the last row and
 * column of tiles are not walked.  GSX_SEM_STD_3DGS: that rule set's exponent, two skips and stop on the packed records,
 * alpha = min(0.99, ..); pixels beyond the frame's width or height are never walked.  w is the very value those entries
 * multiply dL/dpixel with: weight_sum equals grad_colors[:, 0] of gsx_render_backward (gsx_render_backward_std) under
 * dL/dframe = 1 bit for bit.  No float atomics: same inputs, same bits.
 * accumulate == 0: every row of the arrays is written -- the call clears them on `stream` first, so a row the frame did
 * not list reads +0 / 0 -- and views = 1 where listed.  accumulate == 1: a listed row is merged into what the arrays hold
 * (max, +=, +=, views += 1) and an unlisted row is not touched: a sweep over the training views is one call per view.
 * workspace: gsx_contribution_workspace_bytes.
 */
GSX_API int gsx_render_contribution(const GsxCamera *camera, const float *means3d, const float *scales, const float *quats,
                                    const float *opacity_logit, const float *colors, int64_t n, int32_t tile_size,
                                    float *weight_max /* (n) */, float *weight_sum /* (n) */, uint32_t *pixels /* (n) */,
                                    uint32_t *views /* (n), may be NULL */, int32_t accumulate, const GsxParams *params,
                                    void *workspace, size_t workspace_bytes, void *stream);

/* Bytes of device workspace gsx_render_contribution needs (0 on invalid arguments). */
GSX_API size_t gsx_contribution_workspace_bytes(int64_t n, int32_t width, int32_t height, int32_t tile, int64_t max_instances);

/*
 * Replaces Gaussians.get_3d_covariance_matrix (splat/gaussians.py:54-69): covariance_out (n,3,3) =
 * (R S)(R S)^T from linear scales (n,3) and quaternions (n,4) (w,x,y,z), the quaternion
 * normalised twice as the reference does.  The render entry points compute this inline; the
 * function exists for callers of the reference's method.
 */
GSX_API int gsx_covariance_3d(const float *scales, const float *quats, int64_t n, float *covariance_out, void *stream);

/*
 * Replaces GaussianScene.get_2d_covariance (splat/gaussian_scene.py:53-68 -> compute_2d_covariance,
 * splat/utils.py:320-354): the EWA 2D covariance (n,2,2) of caller-given points (n,3) with 3D covariances
 * (n,3,3) under `camera` -- view-space point clamped at 1.3 tan(fov/2), J from the COLMAP focal lengths,
 * (((J W) Sigma) W^T) J^T left to right, top-left 2x2.  No cull: every row is projected.
 */
GSX_API int gsx_covariance_2d(const GsxCamera *camera, const float *points, const float *covariance_3d, int64_t n,
                      float *covariance_2d_out, void *stream);

/*
 * Debug helper on the same projection: replaces GaussianScene.render_points_image
 * (splat/gaussian_scene.py:44-51, splat/image.py:72-89).  Writes (x_pix, y_pix, ndc_z) for every
 * Gaussian in input order into points_out (n,3) and 1/0 into in_view_out (n) (uint8).
 */
GSX_API int gsx_project_points(const GsxCamera *camera, const float *means3d, int64_t n, float *points_out,
                       uint8_t *in_view_out, void *stream);

/*
 * Build extension (no counterpart in the reference, whose colour is the stored rgb/256,
 * splat/gaussians.py:20-22): view-dependent colour from real spherical harmonics of degree 0..3 in
 * the published 3D Gaussian Splatting convention, colour = max(0, 0.5 + sum_k Y_k(d) sh[k]) with
 * d = normalize(mean - camera centre).  sh is (n, (degree+1)^2, 3); camera_center_host is 3 floats
 * in HOST memory (GaussianImage.camera_center, splat/image.py:66); colors_out (n,3) then feeds the
 * `colors` argument of gsx_render_forward.
 */
GSX_API int gsx_sh_to_rgb(const float *means3d, const float *sh, int32_t degree, int64_t n,
                  const float *camera_center_host, float *colors_out, void *stream);

/*
 * Backward of gsx_sh_to_rgb (build extension), the last link of an SH scene's gradient chain: from grad_colors (n,3) =
 * dL/d(view-dependent colour) -- what gsx_render_backward / gsx_render_backward_geometry write when they are handed the
 * colours gsx_sh_to_rgb evaluated -- to grad_sh (n, (degree+1)^2, 3) = dL/dsh and, when grad_means3d is not NULL, to
 * grad_means3d (n,3), the gradient that reaches the mean through the view direction d = v / |v|, v = mean - camera centre:
 *   m_c = 1 where 0.5 + sum_k Y_k(d) sh[k][c] > 0 (the forward's own operations and order), else 0;
 *   grad_sh[i][k][c] = Y_k(d) m_c grad_colors[i][c];
 *   grad_means3d[i]  = (g - d (d . g)) / |v|,  g = sum_k sum_c m_c grad_colors[i][c] sh[k][c] dY_k/dd.
 * Every entry of both outputs is written (exact zeros for a clamped channel, and for grad_means3d at degree 0); grad_means3d
 * is written, not accumulated: a caller that also has gsx_render_backward_geometry's dL/dmeans3d adds the two.  No atomics:
 * same inputs, same bits.  Does not synchronise.  n == 0 is GSX_OK.
 * The zero-row rule: a row whose grad_colors is zero in every channel the forward did not clamp (m_c grad_colors[i][c] = 0
 * for all c) gets exact zeros in grad_sh and grad_means3d, whatever its mean and coefficients hold -- NaN, an infinity, a
 * mean that IS the camera centre (no view direction).  Every Gaussian that is culled or on no tile list is such a row (its
 * grad_colors is 0), so a row a fit has lost reaches neither the coefficients' gradient nor, through the sum of
 * grad_means3d over all rows that the pose gradient of an SH scene takes, dL/dworld2view.  A row with a non-zero masked
 * grad_colors holds the bits it held before the rule.
 */
GSX_API int gsx_sh_backward(const float *means3d, const float *sh, int32_t degree, int64_t n,
                            const float *camera_center_host, const float *grad_colors,
                            float *grad_sh, float *grad_means3d /* may be NULL */, void *stream);

/*
 * The SH degree schedule of a fit (build extension): the two entries above on the first (active_degree + 1)^2 coefficients of
 * rows STORED at stored_degree.  sh and grad_sh are (n, K_S, 3), K_S = (stored_degree + 1)^2; of each row only the
 * coefficients k < K_A = (active_degree + 1)^2 are read -- what the others hold, NaN included, reaches no output.  With
 * P = sh[:, :K_A] made contiguous, bit for bit:
 *   colors_out        = what gsx_sh_to_rgb(P, active_degree) writes;
 *   grad_sh[:, :K_A]  = what gsx_sh_backward(P, active_degree) writes, grad_sh[:, K_A:] = +0 -- every entry is written;
 *   grad_means3d      = what gsx_sh_backward(P, active_degree) writes (may be NULL).
 * active_degree == stored_degree runs the kernels of the two entries above.  Any float-aligned base.  No atomics, does not
 * synchronise, n == 0 is GSX_OK.  A degree outside 0..3 or active_degree > stored_degree: GSX_ERR_INVALID_ARGUMENT before
 * any HIP call, gsx_last_error names the argument.
 */
GSX_API int gsx_sh_to_rgb_active(const float *means3d, const float *sh, int32_t stored_degree, int32_t active_degree,
                                 int64_t n, const float *camera_center_host, float *colors_out, void *stream);
GSX_API int gsx_sh_backward_active(const float *means3d, const float *sh, int32_t stored_degree, int32_t active_degree,
                                   int64_t n, const float *camera_center_host, const float *grad_colors,
                                   float *grad_sh, float *grad_means3d /* may be NULL */, void *stream);

/*
 * Build extension (the reference renders and stops): the photometric loss every splat fit minimises (Kerbl et al. 2023),
 * value and gradient in one call.  image (the frame, x) and target (y) are channel-interleaved (.., .., 3) float32; only
 * the region [0, rows) x [0, cols) of the two leading axes takes part, exactly as if both had been cropped to it -- a row of
 * each starts every *_row_stride floats (>= 3 cols: the caller crops by passing the full image's stride).  The window is
 * symmetric, so GSX_LAYOUT_WH3 and GSX_LAYOUT_HW3 frames are the same problem.
 *   g[i] = exp(-(i - 5)^2 / (2 1.5^2)) / sum, i = 0..10;  G* = the separable 11 x 11 filter per channel, zero padding 5
 *   mu1 = G*x, mu2 = G*y, p = G*(x x), q = G*(x y), r = G*(y y);  s1 = p - mu1^2, s2 = r - mu2^2, s12 = q - mu1 mu2
 *   A1 = 2 mu1 mu2 + C1, A2 = 2 s12 + C2, B1 = mu1^2 + mu2^2 + C1, B2 = s1 + s2 + C2,  C1 = 0.01^2, C2 = 0.03^2
 *   ssim = mean(A1 A2 / (B1 B2)) and l1 = mean|x - y| over the n = 3 rows cols elements
 *   loss = (1 - lambda_dssim) l1 + lambda_dssim (1 - ssim)
 * loss_out (DEVICE, 3 floats) receives loss, l1, ssim.  grad_image (DEVICE, or NULL for the value alone) receives
 * dloss/dimage: with w = -lambda_dssim / n,
 *   Dmu = 2 mu2 (A2 - A1) / (B1 B2) - 2 mu1 A1 A2 (B2 - B1) / (B1 B2)^2,  Dp = -A1 A2 / (B1 B2^2),  Dq = 2 A1 / (B1 B2)
 *   grad = (1 - lambda_dssim) sign(x - y) / n + G*(w Dmu) + 2 x G*(w Dp) + y G*(w Dq),  sign(0) = 0
 * Exactly the rows x cols x 3 region elements are written (a row every grad_row_stride floats, nothing behind a row's
 * 3 cols floats), written, not accumulated, and scaled by nothing but the formula.  Vector accesses are used wherever a
 * base pointer is 16-byte aligned and its stride a multiple of 4 floats; any float-aligned base and stride is accepted.
 * No atomics: same inputs, same bits, and loss_out holds the same bits with and without grad_image.
 * Refused with GSX_ERR_INVALID_ARGUMENT (gsx_last_error names the argument), before any HIP call: NULL image, target,
 * loss_out or workspace; rows or cols <= 0; a stride < 3 cols; lambda_dssim outside [0, 1] or not finite; a region of more
 * than 2^31 - 1 tiles of 32 x 32; a workspace that is not 256-byte aligned.  workspace:
 * gsx_photometric_loss_workspace_bytes(rows, cols, grad_image != NULL); fewer bytes: GSX_ERR_WORKSPACE_TOO_SMALL.
 * Does not synchronise, does not allocate, reads no hints: stream-ordered, may be captured into a hipGraph.
 */
GSX_API int gsx_photometric_loss(const float *image, int64_t image_row_stride, const float *target, int64_t target_row_stride,
                                 int32_t rows, int32_t cols, float lambda_dssim, float *loss_out /* 3 floats */,
                                 float *grad_image /* may be NULL */, int64_t grad_row_stride,
                                 void *workspace, size_t workspace_bytes, void *stream);

/* Bytes of device workspace gsx_photometric_loss needs: one partial-sum pair per tile and, with_grad != 0, the three
 * gradient maps (0 on invalid arguments). */
GSX_API size_t gsx_photometric_loss_workspace_bytes(int32_t rows, int32_t cols, int32_t with_grad);

/*
 * Build extension: the loss above for photographs -- a per-pixel weight m (a mask: sky, passers-by, a matte, the
 * undistortion border) and a per-view exposure E, a 3 x 4 affine colour transform applied to the frame before it meets the
 * target (auto-exposure and white balance differ from shot to shot; the published implementation learns the same term beside
 * the Gaussians).  Symbols as above; sums run over the region's pixels:
 *   x'_i = ((E_i0 x_0 + E_i1 x_1) + E_i2 x_2) + E_i3      each product and sum rounded to float32, in this order;
 *                                                         x' = x when exposure is NULL
 *   outside the region x' is 0, not E_i3: the windows see the two images as if cropped, as above
 *   W    = sum m                                          (rows * cols when weight is NULL)
 *   l1   = sum_pix m sum_ch |x' - y| / (3 W)
 *   ssim = sum_pix m sum_ch (A1 A2 / (B1 B2)) / (3 W)     the SSIM map is formed from x' and y unweighted; m weighs the map
 *   loss = (1 - lambda) l1 + lambda (1 - ssim)
 *   g'   = (1 - lambda) m sign(x' - y) / (3 W) + G*(w m Dmu) + 2 x' G*(w m Dp) + y G*(w m Dq),   w = -lambda / (3 W)
 *   dL/dx      = E[:, :3]^T g'           per region pixel (g' itself when exposure is NULL)
 *   dL/dE[i,j] = sum_pix g'_i x_j (j < 3),  dL/dE[i,3] = sum_pix g'_i
 *   W == 0: loss_out = (0, 0, 0, 0), every gradient an exact +0
 * A pixel with m = 0 still reaches the loss through the windows of its neighbours within 5 pixels: m weighs the SSIM map,
 * it does not hide the pixel from the windows (multiplying the images by m would fit black into the hole).  A caller who
 * wants a hard cut dilates the mask by 5 pixels.
 * weight: DEVICE (rows x cols) float32, a row every weight_row_stride floats (>= cols), or NULL; finite and >= 0 is the
 * caller's contract, nothing checks it.  exposure: DEVICE 12 floats, row-major 3 x 4, or NULL -- device memory, so that a
 * step of the exposure never synchronises.  loss_out (DEVICE, 4 floats) receives loss, l1, ssim, W.  grad_image as above.
 * grad_exposure (DEVICE 12 floats, or NULL) receives dL/dE; it needs exposure and grad_image.
 * With weight == NULL and exposure == NULL the call runs the kernels of gsx_photometric_loss: loss_out[0..2] and grad_image
 * hold the same bits, loss_out[3] = rows * cols.  Otherwise 1 / W is not known while the maps are formed: they are stored
 * unscaled, the one workgroup that sums the per-tile partials in double leaves 1 / (3 W) in the workspace, and the gradient
 * kernel multiplies; W is never read back.  No atomics, every sum in a fixed order: same inputs, same bits (dL/dE included),
 * and loss_out holds the same bits with and without the gradients.
 * Refused with GSX_ERR_INVALID_ARGUMENT before any HIP call: everything gsx_photometric_loss refuses; weight_row_stride <
 * cols when weight is given; grad_exposure without exposure or without grad_image.  workspace:
 * gsx_photometric_loss_weighted_workspace_bytes(rows, cols, grad_image != NULL).  Does not synchronise, does not allocate.
 */
GSX_API int gsx_photometric_loss_weighted(const float *image, int64_t image_row_stride, const float *target,
                                          int64_t target_row_stride, const float *weight /* may be NULL */,
                                          int64_t weight_row_stride, const float *exposure /* may be NULL */, int32_t rows,
                                          int32_t cols, float lambda_dssim, float *loss_out /* 4 floats */,
                                          float *grad_image /* may be NULL */, int64_t grad_row_stride,
                                          float *grad_exposure /* may be NULL */, void *workspace, size_t workspace_bytes,
                                          void *stream);

/* Bytes of device workspace gsx_photometric_loss_weighted needs: what gsx_photometric_loss needs, three partial sums per
 * tile, the scale slot and, with_grad != 0, twelve partial sums of dL/dE per tile (0 on invalid arguments). */
GSX_API size_t gsx_photometric_loss_weighted_workspace_bytes(int32_t rows, int32_t cols, int32_t with_grad);

/*
 * Build extension (the reference has no training loop): one Adam step (Kingma & Ba 2015) over up to GSX_ADAM_MAX_GROUPS
 * parameter arrays of the same n rows -- the arrays of a Gaussian container -- in ONE kernel launch, in place.  What it
 * steps along are the gradients the calls above wrote.  Those are exact zeros for every Gaussian that is culled or on no
 * tile list (gsx_render_backward*: "0 for a Gaussian on no tile list"; gsx_sh_backward multiplies by them), which is what
 * makes GSX_ADAM_SKIP_ZERO_ROWS a visibility test -- as long as the caller adds nothing to them: for an SH scene the
 * Python surface adds gsx_sh_backward's view-direction term to dL/dmeans3d before it sets .grad, and that term is itself
 * zero where dL/dcolour is.
 *
 * Each group g is four DEVICE arrays of (n, width) float32 with contiguous rows: param, grad (read only), exp_avg and
 * exp_avg_sq (the moments, zero before step 1).  Host scalars, computed once per call in double and rounded to float:
 *   c1 = 1 - beta1,  c2 = 1 - beta2,  a_g = lr_g / (1 - beta1^step),  s2 = sqrt(1 - beta2^step)
 * Per element, every float32 operation rounded on its own (no fused multiply-add; divide and sqrt correctly rounded):
 *   g' = g (GSX_ADAM_LINEAR)  or  g p (GSX_ADAM_LOG: the gradient with respect to theta = log p)
 *   m' = beta1 m + c1 g';   v' = beta2 v + (c2 g') g';   d = sqrt(v') / s2 + eps;   u = a_g (m' / d)
 *   p' = p - u (GSX_ADAM_LINEAR)  or  p expf(-u) (GSX_ADAM_LOG)
 * A LOG group is Adam on theta with p = exp(theta), the parametrisation the published method gives the scales, without
 * storing theta: its moments are those of dL/dtheta, a positive parameter stays positive for any finite step, and, as no
 * logarithm is ever taken, a non-positive one keeps its sign (it must be positive to mean anything).
 *
 * GSX_ADAM_SKIP_ZERO_ROWS (the published trainer's sparse Adam): row r is skipped iff every gradient element of row r in
 * every group of the call is +0 or -0 (a NaN is not zero).  A skipped row's param, exp_avg and exp_avg_sq are neither read
 * nor written in any group; a row that is not skipped is updated in all groups, also where its gradient is zero.  The
 * bias corrections use the caller's global `step` for every row.
 *
 * No workspace, no allocation, no synchronisation, no hints, no atomics: same inputs, same bits.  16-byte accesses are used
 * in a group whose four base pointers are 16-byte aligned; any float-aligned base is accepted.  `step` (>= 1, the number
 * of this step) enters through host scalars: a hipGraph that captured the call has it baked in.  n == 0 is GSX_OK.
 * Refused with GSX_ERR_INVALID_ARGUMENT (gsx_last_error names the argument) before any HIP call: groups NULL; n_groups
 * outside 1 .. GSX_ADAM_MAX_GROUPS; n < 0; step < 1; beta1 or beta2 outside [0, 1) or not finite; eps negative or not finite;
 * unknown flags; in a group: width outside 1 .. 2^20, an unknown transform, reserved != 0, lr negative or not finite, and,
 * when n > 0, a NULL pointer.
 */
#define GSX_ADAM_MAX_GROUPS 8
enum { GSX_ADAM_LINEAR = 0, GSX_ADAM_LOG = 1 };
#define GSX_ADAM_SKIP_ZERO_ROWS 1u
typedef struct GsxAdamGroup {
    float *param;
    const float *grad;
    float *exp_avg;
    float *exp_avg_sq; /* each (n, width) float32, rows contiguous */
    int32_t width;
    int32_t transform; /* GSX_ADAM_LINEAR / GSX_ADAM_LOG */
    float lr;
    float reserved;    /* must be 0 */
} GsxAdamGroup;
GSX_API int gsx_adam_step(const GsxAdamGroup *groups /* host */, int32_t n_groups, int64_t n, int64_t step /* >= 1 */,
                          float beta1, float beta2, float eps, uint32_t flags, void *stream);

/*
 * Build extension (the reference has no training loop): adaptive density control, the part of the published 3D Gaussian
 * Splatting trainer (Kerbl et al. 2023) that prunes, clones and splits Gaussians every few hundred steps, in three calls:
 * a statistic that is accumulated after every backward pass, a plan that gives every row one action and every output row
 * its place, and one out-of-place rewrite of every array of the container AND of the optimiser's moments along that plan.
 * Device pointers only, the caller owns all memory, nothing is allocated, no atomics: same inputs, same bits.  Every float32
 * operation below is rounded on its own (no fused multiply-add; divide and sqrt correctly rounded).
 *
 * Two statistics.  gsx_density_accumulate takes the norm of any gradient array the caller names (the Python surface's default
 * passes dL/dpoints, in world units); gsx_density_accumulate_screen takes the published one, the norm of the screen-space mean
 * gradient that gsx_render_backward_screen exports, and gsx_density_plan_screen adds the published prune on the screen radius.
 * Two differences from the published method remain, on purpose:
 *  (1) pruning wins over densifying and a split's children are not examined until the next round (the published order
 *      densifies first and prunes the children in the same round);
 *  (2) rows stay in source order with the new rows BESIDE their parent (the published order appends them at the end):
 *      spatial locality is kept, the order is stable, and one scan places every row.
 *
 * gsx_density_accumulate: grad (n, width) float32, read only; grad_sum (n) float32; seen (n) uint32.  Per row
 *   norm = sqrt(((g0 g0 + g1 g1) + g2 g2) + ...), left to right;
 * if any element of the row is not +0 or -0 (a NaN is not zero): grad_sum[i] += norm and seen[i] += 1.  A row of zeros touches
 * neither array.  Does not synchronise.  n == 0 is GSX_OK.  Refused (GSX_ERR_INVALID_ARGUMENT, gsx_last_error names the
 * argument, before any HIP call): n < 0 or n > 2^30; width outside 1 .. 2^20; when n > 0, grad, grad_sum or seen NULL.
 *
 * gsx_density_accumulate_screen: grad_means2d (n,2) and screen_radius (n) float32 as gsx_render_backward_screen wrote them, read
 * only; grad_sum (n) float32; seen (n) uint32; radius_max (n) float32.  Per row, if screen_radius[i] > 0 (a NaN fails the
 * comparison):
 *   norm = sqrtf(g0 g0 + g1 g1);   grad_sum[i] += norm;   seen[i] += 1;
 *   radius_max[i] = r > radius_max[i] ? r : radius_max[i]          (r = screen_radius[i]; a NaN radius_max[i] stays)
 * otherwise the row touches none of the three.  This differs from gsx_density_accumulate on purpose: a row counts as seen when
 * the frame LISTED it, zero gradient or not (and a NaN gradient is added as it is), because the published denominator counts
 * visibility, not non-zero gradients.  Does not synchronise.  n == 0 is GSX_OK.  Refused, before any HIP call: n < 0 or
 * n > 2^30; when n > 0, grad_means2d, screen_radius, grad_sum, seen or radius_max NULL.
 *
 * gsx_density_plan: one action per row i, the comparisons exactly as written, in float32 (a NaN fails every comparison, so a
 * row whose statistic, scales or opacity are NaN where they are compared is KEEP unless another comparison decides), with
 * smax = max(max(s0, s1), s2), which is NaN when one of the three is:
 *   PRUNE (0 output rows): opacity_logit[i] < prune_logit, or smax > prune_scale;                         otherwise
 *   SPLIT (2 rows): seen[i] > 0 and grad_sum[i] / (float)seen[i] >= grad_threshold and smax > dense_scale;  otherwise
 *   CLONE (2 rows): seen[i] > 0 and grad_sum[i] / (float)seen[i] >= grad_threshold and smax <= dense_scale; otherwise
 *   KEEP  (1 row).
 * scales is (n,3), opacity_logit (n): the LOGIT (under GSX_SEM_REF_CPU the effective opacity is sigmoid(sigmoid(logit)), so a
 * probability threshold would mean different things under different rule sets).  The plan -- the action of every row and
 * the exclusive prefix sum of the output counts: the output rows of row i are [prefix[i], prefix[i] + count[i]) -- is left
 * in `workspace` (gsx_density_workspace_bytes(n) bytes, 256-byte aligned) for gsx_density_apply, with n and the counts in
 * its header.  counts_host (HOST, 4 x int64) receives n_out, n_pruned, n_cloned, n_split; the call synchronises `stream`
 * once, after its last launch.  n == 0 is GSX_OK with four zeros.  Refused: grad_sum, seen, scales, opacity_logit (n > 0),
 * rules, counts_host or workspace NULL; n < 0 or n > 2^30; rules->flags != 0; rules->split_shrink not a positive finite
 * number; a workspace that is not 256-byte aligned; fewer bytes than asked for: GSX_ERR_WORKSPACE_TOO_SMALL.
 *
 * gsx_density_plan_screen: gsx_density_plan with one more way to PRUNE, the published prune of Gaussians that grew too large
 * on screen:   PRUNE: ... or radius_max[i] > prune_radius   (float32; a NaN radius_max[i] fails the comparison, exactly
 * equal is not pruned, prune_radius = +inf never prunes).  radius_max (n) may be NULL: the rule is off, and the workspace and the
 * four counts are gsx_density_plan's byte for byte.  Everything else -- the other rules, the workspace, counts_host, the one
 * synchronisation, the refusals -- is gsx_density_plan's; also refused: a prune_radius that is NaN.  The plan feeds gsx_density_apply.
 *
 * gsx_density_apply: every group g is rewritten from src (n, width) into dst (n_out, width), all groups in one launch:
 *   KEEP:  the row is copied, whatever the role.
 *   CLONE: two rows.  The first continues the source row: copied, whatever the role.  The second is the new Gaussian:
 *          copied, except in a GSX_DENSITY_ZERO_NEW group, where every element is +0.
 *   SPLIT: two new rows, child c = 0, 1.  ZERO_NEW: +0.  COPY and QUATS: copied.  SCALES: s_k / split_shrink.
 *          POINTS: p_k + ((R[k][0] (s0 e0) + R[k][1] (s1 e1)) + R[k][2] (s2 e2)),  e = noise[i][c][0..2],
 *          s the PARENT's scales and R the rotation of the parent's quaternion (w, x, y, z) = q / nrm (four divides),
 *          nrm = sqrt(((qw qw + qx qx) + qy qy) + qz qz); (w, x, y, z) = (1, 0, 0, 0) when !(nrm > 0):
 *            R[0][0] = 1 - 2 (y y + z z)   R[0][1] = 2 (x y - w z)       R[0][2] = 2 (x z + w y)
 *            R[1][0] = 2 (x y + w z)       R[1][1] = 1 - 2 (x x + z z)   R[1][2] = 2 (y z - w x)
 *            R[2][0] = 2 (x z - w y)       R[2][1] = 2 (y z + w x)       R[2][2] = 1 - 2 (x x + y y)
 * noise is DEVICE (n, 2, 3) float32 (standard normal draws; the caller's generator is the caller's determinism) and is read
 * for SPLIT rows only.  ZERO_NEW is for Adam's exp_avg / exp_avg_sq: a survivor keeps its moments' bits, a new Gaussian
 * starts at zero.  source_row (DEVICE, int32 (n_out), may be NULL): i for an output row that continues source row i,
 * -(i + 1) for a new row made from i.  Nothing is read of a pruned row.  16-byte accesses are used where the addresses allow;
 * any float-aligned base is accepted, with the same bits.
 * The call compares n and n_out with the plan's header: it reads 16 bytes back on `stream` and so waits for what was queued
 * there before it (nothing, straight after gsx_density_plan); it does not wait for its own launch.  n_out == 0 or n == 0 is
 * GSX_OK with nothing launched.  Refused, before any HIP call: groups or workspace NULL; n_groups outside
 * 1 .. GSX_DENSITY_MAX_GROUPS; n < 0 or n > 2^30; n_out < 0 or n_out > 2 n; a workspace that is not 256-byte aligned or too
 * small (GSX_ERR_WORKSPACE_TOO_SMALL); in a group: width outside 1 .. 2^20, an unknown role, src or dst NULL (n, n_out > 0),
 * dst == src; more than one POINTS, SCALES or QUATS group; POINTS or SCALES of a width other than 3, QUATS other than 4; a
 * POINTS group without both a SCALES and a QUATS group; noise NULL with a POINTS group.  Refused after the read: n or n_out
 * different from the plan's.
 */
#define GSX_DENSITY_MAX_GROUPS 24
enum { GSX_DENSITY_COPY = 0, GSX_DENSITY_ZERO_NEW = 1, GSX_DENSITY_POINTS = 2, GSX_DENSITY_SCALES = 3, GSX_DENSITY_QUATS = 4 };
typedef struct GsxDensityGroup {
    const float *src; /* (n, width) float32, rows contiguous */
    float *dst;       /* (n_out, width) */
    int32_t width;
    int32_t role;     /* GSX_DENSITY_COPY .. GSX_DENSITY_QUATS */
} GsxDensityGroup;    /* 24 bytes */
typedef struct GsxDensityRules {
    float grad_threshold, dense_scale, prune_logit, prune_scale, split_shrink;
    uint32_t flags;   /* must be 0 */
} GsxDensityRules;
GSX_API int gsx_density_accumulate(const float *grad, int32_t width, int64_t n, float *grad_sum, uint32_t *seen, void *stream);
GSX_API size_t gsx_density_workspace_bytes(int64_t n);   /* 0 on invalid arguments (n < 0 or n > 2^30) */
GSX_API int gsx_density_plan(const float *grad_sum, const uint32_t *seen, const float *scales, const float *opacity_logit,
                             int64_t n, const GsxDensityRules *rules, void *workspace, size_t workspace_bytes,
                             int64_t *counts_host /* 4 */, void *stream);
GSX_API int gsx_density_accumulate_screen(const float *grad_means2d, const float *screen_radius, int64_t n, float *grad_sum,
                                          uint32_t *seen, float *radius_max, void *stream);
GSX_API int gsx_density_plan_screen(const float *grad_sum, const uint32_t *seen, const float *scales, const float *opacity_logit,
                                    const float *radius_max /* may be NULL */, float prune_radius, int64_t n,
                                    const GsxDensityRules *rules, void *workspace, size_t workspace_bytes,
                                    int64_t *counts_host /* 4 */, void *stream);
/* gsx_density_plan_contribution: a plan of KEEP and PRUNE alone from gsx_render_contribution's arrays, in gsx_density_plan's
 * workspace format, so that the unchanged gsx_density_apply rewrites every array from it.  PRUNE iff weight_max[i] <
 * threshold in float32 -- a NaN weight fails the comparison and is kept, a weight exactly equal is kept -- or, with `views`,
 * views[i] == 0 (no view listed the row), whatever its weight.  A NaN or negative threshold is refused; the other
 * refusals, the alignment rule, counts_host = (n_out, n_pruned, 0, 0) and the one synchronisation are gsx_density_plan's. */
GSX_API int gsx_density_plan_contribution(const float *weight_max, const uint32_t *views /* may be NULL */, float threshold,
                                          int64_t n, void *workspace, size_t workspace_bytes, int64_t *counts_host /* 4 */,
                                          void *stream);
GSX_API int gsx_density_apply(const GsxDensityGroup *groups /* host */, int32_t n_groups, int64_t n, int64_t n_out,
                              const float *noise /* (n,2,3), may be NULL without a POINTS group */,
                              int32_t *source_row /* (n_out), may be NULL */, void *workspace, size_t workspace_bytes,
                              void *stream);

/*
 * Build extension: fixed-budget densification, the second standard strategy of the field (3DGS-MCMC, Kheradmand et al. 2024):
 * two per-step calls -- the gradients of the two regularisers, and an opacity-gated noise step on the positions -- and a
 * round of two calls that relocates dead Gaussians onto live ones drawn in proportion to opacity and grows the container
 * towards its budget the same way.  It needs no densification statistic.  Device pointers only, the caller owns all memory,
 * nothing is allocated.  Throughout: opacity is the LOGIT, scales are linear, every array is contiguous float32, n <= 2^30.
 * Every float32 operation below is rounded on its own (no fused multiply-add; divide and sqrt correctly rounded); expf is the
 * device's.  sigma(o) = 1 / (1 + exp(-o)).
 *
 * gsx_mcmc_regularize: the gradients of  lambda_opacity mean_i sigma(o_i) + lambda_scale mean_ic |s_ic|, added in place,
 * one launch (the VALUE of the two terms is not computed).  With co = (float)((double)lambda_opacity / n) and
 * cs = (float)((double)lambda_scale / (3 n)), per row i, in float32:
 *   sg = 1 / (1 + expf(-o_i));   grad_opacity[i] = grad_opacity[i] + co * (sg * (1 - sg));
 *   grad_scales[i][c] = s_ic > 0 ? grad_scales[i][c] + cs : (s_ic < 0 ? grad_scales[i][c] - cs : grad_scales[i][c])
 * (a scale of +-0 or NaN leaves its element's bits).  A lambda of exactly 0 leaves its gradient array untouched, and its
 * two pointers are not looked at.  Does not synchronise.  n == 0 is GSX_OK.  Refused (GSX_ERR_INVALID_ARGUMENT,
 * gsx_last_error names the argument, before any HIP call): n < 0 or n > 2^30; a lambda that is negative or not finite; when
 * n > 0 and the lambda is not 0: opacity or grad_opacity, scales or grad_scales NULL.
 *
 * gsx_mcmc_perturb: points[i] += delta_i in place, one launch; 17 floats read and 3 written per row.  noise is (n,3), standard
 * normal draws of the caller.  Per row, in float32, in this order:
 *   sg = 1 / (1 + expf(-o));   gate = 1 / (1 + expf(-(gate_k * ((1 - sg) - gate_x0))));
 *   nrm = sqrtf(((qw qw + qx qx) + qy qy) + qz qz);   (w, x, y, z) = q / nrm  (four divides; NO fallback for nrm == 0);
 *   R as in gsx_density_apply;
 *   u_c = (R[0][c] e0 + R[1][c] e1) + R[2][c] e2;         (R^T e)
 *   v_c = (s_c s_c) u_c;
 *   d_k = (rate gate) ((R[k][0] v0 + R[k][1] v1) + R[k][2] v2);     (rate * gate is one product, formed first)
 *   if d_0, d_1 and d_2 are all finite: points[i][k] = points[i][k] + d_k; otherwise the row keeps its bits (a zero
 *   quaternion, a NaN in the noise: training does not die of one bad row).
 * That is delta = rate gate Sigma e with Sigma = R diag(s^2) R^T.  The published gate is gate_k = 100, gate_x0 = 0.995, the
 * published rate 5e5 x the position learning rate.  Does not synchronise.  n == 0 is GSX_OK.  Refused: n < 0 or n > 2^30;
 * rate, gate_k or gate_x0 not finite, rate or gate_k negative; when n > 0, any of the five pointers NULL.
 *
 * gsx_mcmc_plan: who is dead, who is drawn, how often -- exact integer arithmetic, a pure function of its inputs.
 *   row i is DEAD when opacity[i] <= dead_logit (float32; a NaN fails it);
 *   weights[i] = dead or opacity[i] not finite ? 0 : max(1, rint(2^22 sigma(o_i)))      (sigma in double);
 *   P = the exclusive prefix sum of the weights in uint64, total = their sum (<= 2^52);
 *   output row j (0 <= j < n_out, n_out >= n) is DRAWN when j >= n (a new row) or row j is dead:
 *     t = min(total - 1, (uint64) floor(uniforms[j] * (double) total))        (one IEEE double multiplication)
 *     source[j] = the unique s with P[s] <= t < P[s] + weights[s];   count[s] += 1   (an integer atomic)
 *   every other row: source[j] = j.  count[s] is 0 for a row nobody drew.
 *   total == 0: every source[j] = min(j, n - 1), every count 0.
 * uniforms is DEVICE (n_out) float64 in [0, 1) (a value outside, or a NaN, is clamped into the range of t); row j reads its
 * own slot only.  weights (n) uint32, source (n_out) int32, count (n) uint32 are written whole.  counts_host (HOST, 3 x
 * int64) receives n_dead, n_live (rows of non-zero weight), n_new = n_out - n; the call synchronises `stream` once, after
 * its last launch.  workspace: gsx_mcmc_workspace_bytes(n) bytes, 256-byte aligned.  n == 0 is GSX_OK with three zeros
 * (n_out must be 0 then).  Refused: n < 0 or n > 2^30; n_out < n or n_out > 2^30; dead_logit NaN; opacity, uniforms, weights,
 * source, count (n > 0), counts_host or workspace NULL; a workspace that is not 256-byte aligned; fewer bytes than asked for:
 * GSX_ERR_WORKSPACE_TOO_SMALL.
 *
 * gsx_mcmc_apply: every group g is rewritten from src (n, width) into dst (n_out, width), all groups in one launch.  For
 * output row j: s = source[j], c = count[s], N = min(c + 1, GSX_MCMC_N_MAX).
 *   N == 1 (then s == j): every group copies the row's bits.
 *   N > 1 (the source row itself and each of its copies alike): GSX_MCMC_COPY: the bits of row s.  GSX_MCMC_ZERO_MOVED (Adam's
 *   moments): +0.  GSX_MCMC_OPACITY (width 1) and GSX_MCMC_SCALES (width 3): the published relocation, in double:
 *     a = min(sigma(o_s), 1 - 2^-24);   x = -expm1(log1p(-a) / N);                          (= 1 - (1 - a)^(1/N))
 *     D = sum_{i=1..N} sum_{k=0..i-1} ((C(i-1,k) (-1)^k) x^(k+1)) / sqrt(k+1), ONE accumulator, i outer, k inner, each term
 *         added as written; C(i-1,0) = 1, C(i-1,k+1) = (C(i-1,k) (i-1-k)) / (k+1) (exact), x^(k+1) by running multiplication;
 *     opacity: the logit log(p / (1 - p)) of p = min(max(x, (double) min_opacity), 1 - 2^-24), rounded to float32;
 *     scales:  (float)((a / D) * (double) s_sc).
 *   The clamp of a keeps the alternating sum away from catastrophic cancellation: its terms are bounded by x (1 + x)^(N-1).
 * A source[j] outside 0 .. n-1 is read as min(j, n - 1) with N = 1: a broken plan stays inside the arrays.  Does not
 * synchronise.  n == 0 or n_out == 0 is GSX_OK with nothing launched.  Refused, before any HIP call: groups, source or count
 * NULL; n_groups outside 1 .. GSX_DENSITY_MAX_GROUPS; n < 0 or n > 2^30; n_out < n or n_out > 2^30; min_opacity outside
 * (0, 1); in a group: width outside 1 .. 2^20, an unknown role, src or dst NULL, dst == src; more than one OPACITY or SCALES
 * group; OPACITY of a width other than 1, SCALES other than 3; a SCALES group without an OPACITY group.
 */
#define GSX_MCMC_N_MAX 51    /* the published n_max: the largest N the relocation is evaluated for */
enum { GSX_MCMC_COPY = 0, GSX_MCMC_ZERO_MOVED = 1, GSX_MCMC_OPACITY = 2, GSX_MCMC_SCALES = 3 };
GSX_API int gsx_mcmc_regularize(const float *opacity /* (n) */, const float *scales /* (n,3) */, int64_t n, float lambda_opacity,
                                float lambda_scale, float *grad_opacity /* (n) */, float *grad_scales /* (n,3) */, void *stream);
GSX_API int gsx_mcmc_perturb(float *points /* (n,3) */, const float *scales /* (n,3) */, const float *quaternions /* (n,4) */,
                             const float *opacity /* (n) */, const float *noise /* (n,3) */, int64_t n, float rate, float gate_k,
                             float gate_x0, void *stream);
GSX_API size_t gsx_mcmc_workspace_bytes(int64_t n);   /* 0 on invalid arguments (n < 0 or n > 2^30) */
GSX_API int gsx_mcmc_plan(const float *opacity /* (n) */, int64_t n, float dead_logit, int64_t n_out,
                          const double *uniforms /* (n_out) */, uint32_t *weights /* (n) */, int32_t *source /* (n_out) */,
                          uint32_t *count /* (n) */, void *workspace, size_t workspace_bytes, int64_t *counts_host /* 3 */,
                          void *stream);
GSX_API int gsx_mcmc_apply(const GsxDensityGroup *groups /* host; role: GSX_MCMC_COPY .. GSX_MCMC_SCALES */, int32_t n_groups,
                           int64_t n, int64_t n_out, const int32_t *source /* (n_out) */, const uint32_t *count /* (n) */,
                           float min_opacity, void *stream);

/*
 * Build extension: scale initialisation.  The reference's Gaussians.initialize_scale (splat/gaussians.py:35-52: the mean of
 * the three smallest neighbour distances; switched off there, its n x n x 3 difference tensor does not fit) as one call that
 * is exact: for every one of n points the distances to its three nearest OTHER points.  Device pointers only, the caller owns
 * all memory, no float atomics: a pure function of `points`, the same bits on every run.  Every float32 operation below is
 * rounded on its own (no fused multiply-add; sqrt and divide correctly rounded).
 *
 * For row i, over all rows j != i (exclusion is by ROW, not by value: a duplicate point counts, at distance 0):
 *   dx = xj - xi, dy = yj - yi, dz = zj - zi;   q = (dx dx + dy dy) + dz dz;
 * the three smallest q, ascending: q0 <= q1 <= q2, and d_k = sqrtf(q_k).  A neighbour that does not exist (n < 4) is +inf.
 * Only the VALUES of the three smallest q enter, so ties need no rule and the result does not depend on the order in which
 * candidates are met.
 *   dist3 (n, 3) float32, may be NULL: d0, d1, d2.
 *   scale (n) float32, may be NULL:
 *     GSX_KNN_RULE_REFERENCE   max(((d0 + d1) + d2) / 3.0f, 1e-5f)          (splat/gaussians.py:46-48)
 *     GSX_KNN_RULE_PUBLISHED   sqrtf(max(((q0 + q1) + q2) / 3.0f, 1e-7f))   (the linear scale of the published 3D Gaussian
 *                              Splatting initialisation: the root of the mean squared distance)
 * points is (n, 3) float32 and is only read.  FINITE coordinates are a precondition: with a NaN or an infinity the values of
 * the rows are unspecified, but the call still ends and stays inside its arrays.
 * order (DEVICE, int32 (n), may be NULL: rows as given): a permutation of 0 .. n-1, the sequence in which rows are grouped
 * into blocks of 256 for the search.  It changes the speed -- blocks of a space-filling curve are compact, and whole blocks
 * are skipped by an exact lower bound of their distances -- and never a bit of the result.  (An entry that is not a row is
 * replaced by its own position; with an `order` that is not a permutation the rows' values are unspecified.)
 * candidates (HOST, may be NULL): the number of (query, candidate) pairs whose q was evaluated; n (n - 1) without pruning.
 * The call synchronises `stream` only when candidates is asked for.  workspace: gsx_knn3_workspace_bytes(n) bytes, 256-byte
 * aligned (16 n bytes of gathered points, 32 bytes per block, a header).
 * n == 0 is GSX_OK, nothing is written or looked at.  Refused (GSX_ERR_INVALID_ARGUMENT, gsx_last_error names the argument,
 * before any HIP call): n < 0 or n > 2^30; an unknown rule; dist3 and scale both NULL; when n > 0: points NULL, workspace NULL
 * or not 256-byte aligned; fewer workspace bytes than asked for: GSX_ERR_WORKSPACE_TOO_SMALL.
 */
enum { GSX_KNN_RULE_REFERENCE = 0, GSX_KNN_RULE_PUBLISHED = 1 };
GSX_API size_t gsx_knn3_workspace_bytes(int64_t n);   /* 0 on invalid arguments (n < 0 or n > 2^30) */
GSX_API int gsx_knn3(const float *points /* (n,3) */, int64_t n, const int32_t *order /* (n), may be NULL */, int32_t rule,
                     float *dist3 /* (n,3), may be NULL */, float *scale /* (n), may be NULL */,
                     int64_t *candidates /* host, may be NULL */, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Build extension: a similarity transform of the world, x' = s R x + t (R a proper rotation, s > 0), applied IN PLACE to the
 * arrays of a Gaussian container in ONE kernel launch -- the means, the linear scales, the quaternions and, for an SH
 * container, every stored band of the coefficients, rotated so that the colour seen from the transformed camera centre
 * along R d is the colour that was seen along d.  Opacities and RGB colours do not change and are not arguments.
 *
 * The HOST passes everything ready-made in a GsxTransform, all float32 (row-major matrices): R, s, t, the quaternion q_R of R
 * (w, x, y, z) and the SH rotation matrices M1 (3 x 3), M2 (5 x 5), M3 (7 x 7) of bands 1..3 in the basis of gsx_sh_to_rgb
 * (its constants and signs), defined by  Y_l(R d)^T M_l c = Y_l(d)^T c  for every unit d.  The kernel derives nothing from
 * anything: its output is a pure function of its arguments.  (That q_R and M_l belong to R is the caller's business and is
 * not checked; the Python surface computes them in float64, intro_to_gaussian_splatting_amd/transform.py.)
 *
 * Per row, every float32 operation rounded on its own (no fused multiply-add), in exactly this order:
 *   points       (x, y, z) -> p'_k = s ((R[k][0] x + R[k][1] y) + R[k][2] z) + t[k]                              k = 0..2
 *   scales       c'_k = s c_k                                                                                   k = 0..2
 *   quaternions  q' = q_R (x) q, the Hamilton product, a = q_R, b = q, components (w, x, y, z) as in the R[i][j] table above
 *                (gsx_density_apply) -- NOT renormalised: a unit q_R keeps |q|, and the renderer normalises as it always does:
 *                  w' = ((a.w b.w - a.x b.x) - a.y b.y) - a.z b.z
 *                  x' = ((a.w b.x + a.x b.w) + a.y b.z) - a.z b.y
 *                  y' = ((a.w b.y - a.x b.z) + a.y b.w) + a.z b.x
 *                  z' = ((a.w b.z + a.x b.y) - a.y b.x) + a.z b.w
 *   sh           (n, (sh_degree + 1)^2, 3).  For every band l = 1 .. sh_degree (ALL stored bands: an SH degree schedule's
 *                inactive bands too), m = 2 l + 1, o = l^2, each channel c, each i = 0 .. m-1:
 *                  sh'[o + i][c] = (..((M_l[i][0] sh[o][c] + M_l[i][1] sh[o + 1][c]) + M_l[i][2] sh[o + 2][c]) + ..)
 *                                  + M_l[i][m - 1] sh[o + m - 1][c]         (the m products summed left to right)
 *                Band 0 is neither read nor written.  A band of zeros stays zero (of either sign).
 * sh == NULL with sh_degree == 0 is an RGB container; sh is not looked at when sh_degree == 0.
 *
 * A workgroup owns 256 consecutive rows (the block of gsx_adam_step and GsxParams.block_bounds) and stages their coefficient
 * run through LDS, with 16-byte accesses when `sh` is 16-byte aligned and float by float otherwise: any float-aligned base is
 * accepted, WITH THE SAME BITS.  No workspace, no allocation, no synchronisation, no atomics.  n == 0 is GSX_OK.
 * Refused with GSX_ERR_INVALID_ARGUMENT (gsx_last_error names the argument) before any HIP call: n < 0 (or more than 2^31 - 1
 * blocks); sh_degree outside 0..3; transform NULL; an entry of the transform that is not finite; s <= 0; when n > 0: points,
 * scales or quaternions NULL, sh NULL with sh_degree > 0.
 */
typedef struct GsxTransform {
    float R[9];   /* row-major: R[3 i + j] */
    float s;
    float t[3];
    float q_R[4]; /* (w, x, y, z) */
    float M1[9];  /* row-major, like M2 and M3 */
    float M2[25];
    float M3[49];
} GsxTransform;   /* 100 floats */
GSX_API int gsx_transform_gaussians(float *points /* (n,3) */, float *scales /* (n,3) */, float *quaternions /* (n,4) */,
                                    float *sh /* (n, (sh_degree+1)^2, 3), may be NULL when sh_degree == 0 */, int32_t sh_degree,
                                    int64_t n, const GsxTransform *transform /* host */, void *stream);

/*
 * Build extension: photo rectification.  One photograph (uint8 RGB, as a decoder leaves it) is resampled, under the lens
 * model COLMAP estimated for it, into the pinhole camera a rule set renders: the float32 target a fit compares its frames
 * with, and the per-pixel weight of gsx_photometric_loss_weighted (1 where the photo covers the pixel, 0 on the
 * undistortion border).  Box-filtered over S x S sub-samples (S = samples) so that a multi-megapixel photo can be brought
 * down to the training size without aliasing.  ONE kernel launch, one thread per output pixel; no workspace, no
 * synchronisation, no atomics, no hints: a pure function of its arguments, the same bits on every run.
 *
 * lens   (HOST) the photo's camera: COLMAP's model id, size and params in COLMAP's order --
 *          GSX_LENS_SIMPLE_PINHOLE f, cx, cy            GSX_LENS_PINHOLE fx, fy, cx, cy
 *          GSX_LENS_SIMPLE_RADIAL  f, cx, cy, k         GSX_LENS_RADIAL  f, cx, cy, k1, k2
 *          GSX_LENS_OPENCV         fx, fy, cx, cy, k1, k2, p1, p2
 *        (f: fx_s = fy_s = f; a coefficient the model lacks is 0).  COLMAP's image coordinates: the centre of pixel 0 is
 *        at 0.5.  The fisheye models, FOV and FULL_OPENCV (ids 5..10) are refused by name with GSX_ERR_UNSUPPORTED.
 * target (HOST) the pinhole to resample to, in OUTPUT PIXEL-INDEX coordinates (index i sits at i): the view-space direction
 *        of index (i, j) is ((i - cx) / fx, (j - cy) / fy, 1).  Which (fx, cx) a rule set's frame has for a given camera is
 *        the caller's business (intro_to_gaussian_splatting_amd/capture.py: rectified_camera).
 * photo  (DEVICE) (lens.height, lens.width, 3) bytes, rows photo_row_stride bytes apart, only read.
 * image_out (DEVICE) (target.width, target.height, 3) float32, the frame's default layout GSX_LAYOUT_WH3; weight_out
 *        (DEVICE, may be NULL) (target.width, target.height) float32.  Every element of both is written.
 *
 * Per output pixel (i, j), every float32 operation rounded on its own (no fused multiply-add; divide correctly rounded), in
 * exactly this order; sub-samples b = 0 .. S-1 (outer, along y), a = 0 .. S-1 (inner, along x):
 *   y  = (((float) j + (((float) b + 0.5f) / (float) S - 0.5f)) - cy) / fy
 *   x  = (((float) i + (((float) a + 0.5f) / (float) S - 0.5f)) - cx) / fx
 *   xx = x x;  yy = y y;  xy = x y;  r2 = xx + yy;  rho = (k1 + k2 r2) r2                     (= k1 r^2 + k2 r^4)
 *   xd = ((x + x rho) + (2 p1) xy) + p2 (r2 + 2 xx)
 *   yd = ((y + y rho) + p1 (r2 + 2 yy)) + (2 p2) xy
 *   g  = 1 + rho;  gp = k1 + (2 k2) r2                                                        (gp = d rho / d r2)
 *   jxx = ((g + (2 xx) gp) + (2 p1) y) + (6 p2) x;   jyy = ((g + (2 yy) gp) + (6 p1) y) + (2 p2) x
 *   jxy = ((2 xy) gp + (2 p1) x) + (2 p2) y;          det = jxx jyy - jxy jxy     (the Jacobian of (x, y) -> (xd, yd))
 *   u  = fx_s xd + (cx_s - 0.5f);   v = fy_s yd + (cy_s - 0.5f)                    (source INDEX coordinates)
 *   valid:  0 <= u <= W_s - 1  and  0 <= v <= H_s - 1  (all four bilinear taps inside the photo)  and  det > 0 (the
 *           model has not folded back, as a barrel lens does far outside its field); a NaN is not valid.
 *   a valid sample:  x0 = floor(u), x1 = min(x0 + 1, W_s - 1), tx = u - (float) x0, the same along y; per channel, with
 *           the four bytes converted to float:  top = p00 + tx (p01 - p00);  bot = p10 + tx (p11 - p10);
 *           value = top + ty (bot - top);  sum_c = sum_c + value (in sample order);  count = count + 1
 *   image_out[i][j][c] = sum_c / (255.0f (float) count), or +0 when count == 0;  weight_out[i][j] = (float) count / (float)(S S)
 * With the pinhole models every coefficient is 0: xd = x and det = 1 exactly.
 *
 * Refused (gsx_last_error names the argument) before any HIP call, GSX_ERR_INVALID_ARGUMENT unless stated: photo, lens,
 * target or image_out NULL; samples outside 1..8; a size of either camera outside 1 .. 65536; photo_row_stride below
 * 3 lens.width; an unsupported model (GSX_ERR_UNSUPPORTED) or an unknown one; a focal length of either side that is not
 * positive and finite; a lens parameter the model reads, or a target principal point, that is not finite.
 */
enum { GSX_LENS_SIMPLE_PINHOLE = 0, GSX_LENS_PINHOLE = 1, GSX_LENS_SIMPLE_RADIAL = 2, GSX_LENS_RADIAL = 3, GSX_LENS_OPENCV = 4 };
typedef struct GsxLens {
    int32_t model;        /* GSX_LENS_*: COLMAP's camera model id */
    int32_t width, height;
    float params[8];      /* COLMAP's params in COLMAP's order; entries the model does not have are not read */
} GsxLens;
typedef struct GsxPinhole {
    int32_t width, height;
    float fx, fy, cx, cy; /* output pixel-index coordinates: index i sits at i */
} GsxPinhole;
GSX_API int gsx_rectify_photo(const uint8_t *photo /* device, (lens.height, lens.width, 3) */, int64_t photo_row_stride,
                              const GsxLens *lens /* host */, const GsxPinhole *target /* host */, int32_t samples /* 1..8 */,
                              float *image_out /* device (W', H', 3) */, float *weight_out /* device (W', H'), may be NULL */,
                              void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GSX_H_ */
