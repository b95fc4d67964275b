// C ABI of libgsx.so (see include/gsx.h): argument validation, workspace carving and the
// stream-ordered launch sequence.  No device memory is allocated here and nothing is retained
// between calls; errors are returned as codes with a thread-local message.
#include <float.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <initializer_list>

#include "gsx_internal.h"
#ifdef GSX_TEST_HOOKS
#include "gsx_debug.h"
#endif

namespace {

thread_local char g_error[512] = "";

int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof g_error, fmt, ap);
    va_end(ap);
    return code;
}

#define GSX_HIP(expr)                                                                               \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess)                                                                       \
            return fail(GSX_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

using namespace gsx;
using namespace gsx::plan;   // Carve, Plan, carve(), capacity_for(), make_plan(), make_clear_plan(): gsx_plan.h

// Optional per-stage timing with HIP events on the launch stream (GSX_FLAG_TIMING).
struct StageTimer {
    bool on = false;
    hipStream_t s = nullptr;
    hipEvent_t ev[6];
    int n = 0;
    void begin(bool enable, hipStream_t stream) {
        on = enable;
        s = stream;
        mark();
    }
    void mark() {
        if (!on || n >= 6) return;
        if (hipEventCreate(&ev[n]) != hipSuccess) { on = false; return; }
        (void)hipEventRecord(ev[n], s);
        ++n;
    }
    // marks: 0 start | 1 project (+keys) | 2 depth sort | 3 scan | 4 bin | 5 blend
    void finish(GsxFrameStats *st) {
        if (n > 0) (void)hipEventSynchronize(ev[n - 1]);
        if (st) {
            for (int i = 0; i < 6; ++i) st->stage_ms[i] = 0.0f;
            for (int i = 1; i < n; ++i) {
                float ms = 0.0f;
                (void)hipEventElapsedTime(&ms, ev[i - 1], ev[i]);
                st->stage_ms[i - 1] = ms;
            }
            if (n > 1) {
                float ms = 0.0f;
                (void)hipEventElapsedTime(&ms, ev[0], ev[n - 1]);
                st->stage_ms[GSX_STAGE_TOTAL] = ms;
            }
        }
        for (int i = 0; i < n; ++i) (void)hipEventDestroy(ev[i]);
        n = 0;
    }
    ~StageTimer() { finish(nullptr); }
};

int make_plan_or_fail(int32_t width, int32_t height, int32_t tile, float *out_image, const GsxParams *params, Plan &p) {
    char msg[256];
    const int rc = make_plan(width, height, tile, out_image, params, p, msg, sizeof msg);
    return rc == GSX_OK ? GSX_OK : fail(rc, "%s", msg);
}

// n, the input arrays and GsxParams.original_index / row_of_index of the whole-path entry points.
int check_inputs(const Plan &p, int64_t n, const float *means3d, const float *scales, const float *quats,
                 const float *opacity_logit, const float *colors) {
    if (n < 0 || n >= (int64_t)1 << 31) return fail(GSX_ERR_INVALID_ARGUMENT, "n = %lld out of range", (long long)n);
    if (n > 0 && (!means3d || !scales || !quats || !opacity_logit || (!colors && !p.sh)))
        return fail(GSX_ERR_INVALID_ARGUMENT, "an input array is NULL");
    if (p.original_index && !p.row_of_index) return fail(GSX_ERR_INVALID_ARGUMENT, "original_index needs row_of_index (its inverse)");
    return GSX_OK;
}

// backward: the carve mode (gsx_plan.h: kCarveBackward = gsx_render_backward's workspace, kCarveGeometry = gsx_render_backward_geometry's).
int check_workspace(void *workspace, size_t bytes, int64_t n, int64_t max_tiles, Carve &c, int64_t &cap, int backward = kCarveForward) {
    if (!workspace) return fail(GSX_ERR_INVALID_ARGUMENT, "workspace is NULL");
    if ((reinterpret_cast<uintptr_t>(workspace) & 255u) != 0) return fail(GSX_ERR_INVALID_ARGUMENT, "workspace must be 256-byte aligned");
    cap = capacity_for(bytes, n, max_tiles, backward);   // never above 2^31 - 1 pairs, whatever the buffer size
    if (cap < 0)
        return fail(GSX_ERR_WORKSPACE_TOO_SMALL, "workspace of %zu bytes cannot hold %lld Gaussians", bytes, (long long)n);
    c = carve(n, cap, max_tiles, binning_temp_bytes(n, cap), backward);
    return GSX_OK;
}

// The workspace of an entry whose size function gives the one size it takes (the losses, density, MCMC, kNN): `need` of
// them; size_call, formatted with what follows it: that function's call as the message spells it.
int check_sized_workspace(const void *workspace, size_t bytes, size_t need, const char *size_call, ...) {
    if (!workspace) return fail(GSX_ERR_INVALID_ARGUMENT, "workspace is NULL");
    if ((reinterpret_cast<uintptr_t>(workspace) & 255u) != 0) return fail(GSX_ERR_INVALID_ARGUMENT, "workspace must be 256-byte aligned");
    if (bytes >= need) return GSX_OK;
    char call[128];
    va_list ap;
    va_start(ap, size_call);
    vsnprintf(call, sizeof call, size_call, ap);
    va_end(ap);
    return fail(GSX_ERR_WORKSPACE_TOO_SMALL, "workspace of %zu bytes, %s = %zu", bytes, call, need);
}

// gsx_workspace_bytes / gsx_backward_workspace_bytes / gsx_backward_geometry_workspace_bytes: 0 for sizes no call accepts.
size_t workspace_bytes(int64_t n, int32_t width, int32_t height, int32_t tile, int64_t max_instances, int backward) {
    if (n < 0 || width <= 0 || height <= 0 || tile <= 0 || max_instances < 0) return 0;
    if (n >= (int64_t)1 << 31 || max_instances >= (int64_t)1 << 31) return 0;
    return carve(n, max_instances, max_tiles_of(width, height, tile), binning_temp_bytes(n, max_instances), backward).total;
}

// The frame's use of GsxParams.hints (all null / false without a hints buffer).
struct FrameHints {
    gsx::BlendHints blend = gsx::BlendHints{nullptr, nullptr, nullptr, nullptr, 0u};
    const uint32_t *sched = nullptr;   // hints.sched, put together from the previous frame's list lengths, or null
    uint32_t *sched_region = nullptr;  // the hints buffer's schedule region (whether or not it holds a schedule yet), or null
};

// ---- The stage chain of a whole-path frame, up to the tile lists.  gsx_render_backward runs these same functions on the
// same inputs -- without the hints buffer, which never changes a list -- so its tile lists are the forward frame's.

// The depth-sort route, the projection (depth keys, records and tile rectangles by row) and the sampled or LSD depth sort
// (the rectangles by rank).  fh: filled in with the frame's use of GsxParams.hints; nullptr: the buffer is neither read
// nor written.  tm: nullptr = no stage marks.  On return order[r] = the row of depth rank r; sampled: a sampled route
// left the emission's chunk sums.
int project_and_sort(const Plan &p, const Carve &c, char *ws, const GsxCamera &camera, const gsx::GaussiansIn &in,
                     int64_t n, int64_t cap, FrameHints *fh, StageTimer *tm, hipStream_t s, const uint32_t *&order,
                     bool &sampled) {
    uint32_t *k0 = (uint32_t *)(ws + c.keys0), *k1 = (uint32_t *)(ws + c.keys1);
    uint32_t *v0 = (uint32_t *)(ws + c.vals0), *v1 = (uint32_t *)(ws + c.vals1);
    uint32_t *counters = (uint32_t *)(ws + c.counters);
    const uint32_t *row_of = p.original_index ? (const uint32_t *)p.row_of_index : nullptr;
    // GsxParams.hints: what the previous frame of this view left (splitters, tile-list lengths) and what this one
    // leaves.  Only where every producer and consumer exists: the tile-16 REF_CPU compositing kernel (lengths,
    // ranked samples), the 256-bucket depth sort (splitters; the LSD passes of larger scenes only take the schedule).
    const gsx::DepthRoute route = gsx::depth_sort_route(n, p.kept_hint);
    sampled = route != gsx::kDepthLsd;
    gsx::SortHints sh{nullptr, nullptr, nullptr, false};
    gsx::ScheduleHint sched_hint{nullptr, nullptr, nullptr, 0u};
    if (fh && p.hints && (route == gsx::kDepth256 || route == gsx::kDepthLsd) && n >= gsx::kSortSamples && p.grid.count() > 0 &&
        gsx::blend_splits_long_tiles(p.grid, p.semantics, p.generic)) {
        const gsx::HintsLayout hl = gsx::hints_layout(max_tiles_of(p.grid.width, p.grid.height, p.grid.tile),
                                                      max_axis_tiles_of(p.grid.width, p.grid.height, p.grid.tile));
        uint32_t *hdr = (uint32_t *)p.hints;
        // (the LSD passes of larger scenes have no use for splitters, but they leave the sample all the same: the next
        // frame of the view may take the 256-bucket route -- a rank's strip does once its kept count is known)
        sh = gsx::SortHints{hdr, (const uint32_t *)(p.hints + hl.splitters), (uint32_t *)(p.hints + hl.samples),
                            p.hints_valid && route == gsx::kDepth256};
        // the 256-bucket route leaves the next frame's splitters itself -- the exact quantiles of this frame's keys (bucket_sort_kernel)
        // -- and the compositing launch has no sample to rank; the LSD route still leaves a sample for it
        const bool exact = route == gsx::kDepth256 && gsx::knob("GSX_EXACT_SPLITTERS", 1) != 0;
        if (exact) sh.next_splitters = (uint32_t *)(p.hints + hl.splitters);
        fh->blend = gsx::BlendHints{hdr, exact ? nullptr : sh.samples, (uint32_t *)(p.hints + hl.splitters), (uint32_t *)(p.hints + hl.lens), 0u};
        fh->sched_region = (uint32_t *)(p.hints + hl.sched);
        // the schedule costs nothing here (a spare workgroup of the projection launch): every window of more than two
        // tiles per SIMD gets one, unless told not to
        if (p.hints_valid && p.schedule != 0 && p.grid.count() > 2048) {
            sched_hint = gsx::ScheduleHint{(const uint32_t *)(p.hints + hl.lens), (uint32_t *)(p.hints + hl.sched), hdr,
                                           (uint32_t)p.grid.count(), (uint32_t)p.grid.nwy()};
            fh->sched = sched_hint.sched;
        }
    }
    // no splitters on file (a view's first frame, a caller without a hints buffer): the projection launch ranks a sample itself
    gsx::SampleHint presample;
    if (sampled && !sh.use && gsx::knob("GSX_PRESAMPLE", 1) != 0)
        presample = gsx::depth_presample(route, ws + c.temp, n, gsx::emit_chunk_sums(ws + c.temp, n, cap), row_of);
    GSX_HIP(gsx::launch_project_pack(camera, p.camera_device, in, n, p.grid, p.semantics, p.tight, p.antialiased, p.small_batch, p.sh_degree, k0, (gsx::Record *)(ws + c.rec),
                                     (gsx::TileRect *)(ws + c.rect), counters,
                                     p.semantics != GSX_SEM_STD_3DGS ? (float4 *)(ws + c.bbox) : nullptr, sched_hint,
                                     c.temp_bytes >= (size_t)(n / GSX_BOUNDS_ROWS + 1) ? (uint8_t *)(ws + c.temp) : nullptr, s, presample));
    if (tm) tm->mark();  // 1: project (+ depth keys)
    // the sampled routes also leave the per-chunk tile counts the pair emission starts from (one kernel less)
    if (sampled)
        GSX_HIP(gsx::sort_depth_sampled(route, ws + c.temp, k0, k1, v0, v1, n, p.kept_hint, counters + kCtrKept,
                                        counters + kCtrCulled, (const gsx::TileRect *)(ws + c.rect),
                                        (gsx::TileRect *)(ws + c.rrect), 0, gsx::emit_chunk_sums(ws + c.temp, n, cap), sh, s, row_of,
                                        presample.splitters != nullptr));
    else {
        // the LSD passes carry the rectangles along, packed into 4 bytes, when tile coordinates fit 8 bits; the two
        // arrays they travel in are the pair lists' value arrays, which nothing uses before the emission
        const bool carry = p.grid.ntx <= 256 && p.grid.nty <= 256 && cap >= n && gsx::knob("GSX_LSD_CARRY", 1) != 0;
        GSX_HIP(gsx::sort_depth_compact(ws + c.temp, k0, k1, v0, v1, n, counters + kCtrKept, counters + kCtrCulled,
                                        (const gsx::TileRect *)(ws + c.rect), (gsx::TileRect *)(ws + c.rrect), s, sh.samples,
                                        carry ? (uint32_t *)(ws + c.tvals0) : nullptr,
                                        carry ? (uint32_t *)(ws + c.tvals1) : nullptr, row_of));
    }
    if (tm) tm->mark();  // 2: depth sort (drops what reaches no tile, leaves the rectangles in rank order)
    order = v0;
    return GSX_OK;
}

// The pair lists from the rank-ordered rectangles (order, m_dev: see bin_and_blend): the emission, which leaves the
// frame's counts in bc, then -- unless the window is empty -- the stable tile sort: ranges = every tile's [first, last)
// (long tiles flagged as lt says), sorted_vals = the rows of the sorted pairs.  tm: nullptr = no stage mark.
int bin_pairs(const Plan &p, const Carve &c, char *ws, int64_t n, int64_t cap, const gsx::TileRect *rrect,
              const uint32_t *order, const uint32_t *m_dev, bool sums_ready, const gsx::BinCounts &bc,
              const gsx::LongTiles &lt, StageTimer *tm, hipStream_t s, const uint32_t *&sorted_vals) {
    uint2 *ranges = (uint2 *)(ws + c.ranges);
    GSX_HIP(gsx::emit_instances(ws + c.temp, rrect, order, m_dev, n, cap, p.grid, ws + c.tkeys0, (uint32_t *)(ws + c.tvals0),
                                ranges, bc, sums_ready, p.kept_hint, s));
    if (tm) tm->mark();  // 3: scan + emit
    if (p.grid.count() > 0)
        GSX_HIP(gsx::sort_instances(ws + c.temp, cap, p.grid, ws + c.tkeys0, ws + c.tkeys1, (uint32_t *)(ws + c.tvals0),
                                    (uint32_t *)(ws + c.tvals1), ranges, bc.d32, lt, &sorted_vals, s));
    return GSX_OK;
}

// The synchronous read-back: counts = (n_visible, D, M) (zeros unless on_device) and, if redo is given, n_redo's device
// word; then D > cap -- pairs were dropped -- is GSX_ERR_WORKSPACE_TOO_SMALL, with the counts valid all the same.
int read_counts(const Carve &c, char *ws, int64_t cap, bool on_device, uint32_t *redo, int64_t (&counts)[3], hipStream_t s) {
    counts[0] = counts[1] = counts[2] = 0;
    if (on_device) GSX_HIP(hipMemcpyAsync(counts, ws + c.counters + 16, 24, hipMemcpyDeviceToHost, s));
    if (redo) GSX_HIP(hipMemcpyAsync(redo, ws + c.redo, 4, hipMemcpyDeviceToHost, s));
    GSX_HIP(hipStreamSynchronize(s));
    if (counts[1] > cap)
        return fail(GSX_ERR_WORKSPACE_TOO_SMALL, "frame needs %lld tile instances, workspace holds %lld",
                    (long long)counts[1], (long long)cap);
    return GSX_OK;
}

// Steps shared by both render entry points once records and rank-ordered tile rectangles exist.  The pair lists
// (bin_pairs) and the count read-back (read_counts) are the ones gsx_render_backward runs: it runs the forward's own chain.
// `order` = Gaussian index of each depth rank (nullptr: rows are already in compositing order);
// `m_dev` = number of ranks on the device (nullptr: n); `culled_dev` = Gaussians behind the cull plane.
// The pair count D never has to reach the host for the frame to be enqueued: the kernels read
// it from device memory and their grids are sized by the workspace capacity.  The normal call
// synchronises ONCE, after the last launch, to report the counts and to detect D > capacity;
// GSX_FLAG_NO_SYNC skips even that (the counts then arrive in pinned memory on their own).
int bin_and_blend(const Plan &p, const Carve &c, char *ws, int64_t n, int64_t cap, const gsx::TileRect *rrect,
                  const uint32_t *order, const uint32_t *m_dev, const uint32_t *culled_dev, bool sums_ready,
                  GsxFrameStats *stats, StageTimer &tm, hipStream_t s, const FrameHints &fh = FrameHints()) {
    uint32_t *counters = (uint32_t *)(ws + c.counters);
    int64_t *dev2 = (int64_t *)(counters + 4);
    uint2 *ranges = (uint2 *)(ws + c.ranges);
    bool counts_on_device = false, counts_in_host = false;
    bool redo_counted = false;      // the compositing launch counts tiles with reference-order records: GsxFrameStats.n_redo
    const bool has_redo = p.stats_bytes >= offsetof(GsxFrameStats, n_redo) + sizeof(int64_t);
    if (p.plain && !stats) return fail(GSX_ERR_INVALID_ARGUMENT, "GSX_FLAG_PLAIN_FOOTPRINTS needs stats_host: n_redo must reach the caller");
    bool parts_marked = false;      // GsxParams.substrip_events recorded (every path records them once, behind its last launch at the latest)
    // no Gaussians: every tile's list is empty -- GsxParams.tile_counts says so (an empty WINDOW has no entries)
    if (n == 0 && p.tile_counts && p.grid.count() > 0)
        GSX_HIP(gsx::launch_zero_words(p.tile_counts, (size_t)p.grid.count(), s));
    if (p.grid.count() > 0 && n == 0 && p.semantics == GSX_SEM_STD_3DGS) {
        // no Gaussians: every pixel of the window is the background colour
        tm.mark();  // 3: scan + emit
        GSX_HIP(gsx::launch_zero_words((uint32_t *)ranges, (size_t)p.grid.count() * 2, s));
        GSX_HIP(gsx::launch_blend((const gsx::Record *)(ws + c.rec), nullptr, (const uint32_t *)(ws + c.tvals0), ranges,
                                  p.grid, p.out, p.semantics, p.background, p.generic, make_clear_plan(p, false),
                                  gsx::LongTiles{nullptr, nullptr, 0u}, nullptr, gsx::BlendHints{nullptr, nullptr, nullptr, nullptr, 0u}, s));
    } else if (n == 0) {
        tm.mark();
        GSX_HIP(gsx::launch_clear(make_clear_plan(p, true), p.out.ptr, s));
    } else {
        // the counts are produced by the emit kernel even when no tile is rendered (an empty window
        // still reports n_visible; its pair count is 0 because every rectangle was clamped away)
        gsx::BinCounts bc{dev2, nullptr, counters + kCtrPairs, counters + kCtrLong, (uint32_t *)(ws + c.redo), culled_dev, n};
        if (p.no_sync && stats) {
            // pinned host memory is device-visible: the emit kernel stores the two counts there itself
            void *alias = nullptr;
            if (hipHostGetDevicePointer(&alias, stats, 0) == hipSuccess && alias) {
                bc.stats2_host = (int64_t *)alias;
                counts_in_host = true;
            } else {
                (void)hipGetLastError();
            }
        }
        const bool split = p.split && cap > 0 && gsx::blend_splits_long_tiles(p.grid, p.semantics, p.generic);
        gsx::LongTiles lt{counters + kCtrLong, (uint32_t *)(ws + c.longs), split ? gsx::kMaxLongTiles : 0u};
        lt.redo = (uint32_t *)(ws + c.redo);
        if (fh.blend.lens) {        // GsxParams.hints: the tiles' costs decide who is long (tile_ranges_kernel)
            lt.cost = fh.blend.lens;
            lt.header = fh.blend.header;
            lt.cost_pct = (uint32_t)gsx::knob("GSX_LONG_COST_PCT", 30);      // (test library only)
            lt.stay_pct = (uint32_t)gsx::knob("GSX_LONG_STAY_PCT", 75);
            if (!fh.sched || lt.cost_pct == 0) lt.header = nullptr;
        }
        const uint32_t *sorted_vals = nullptr;
        const int rc = bin_pairs(p, c, ws, n, cap, rrect, order, m_dev, sums_ready, bc, lt, &tm, s, sorted_vals);
        if (rc != GSX_OK) return rc;
        counts_on_device = true;
        if (p.grid.count() == 0) {
            GSX_HIP(gsx::launch_clear(make_clear_plan(p, true), p.out.ptr, s));
        } else {
            if (p.tile_counts) GSX_HIP(gsx::launch_tile_counts(ranges, p.grid.count(), p.tile_counts, s));
            const uint32_t *sched = fh.sched;      // handed over by the previous frame (GsxParams.hints): no kernel
            gsx::BlendHints bh = fh.blend;
            bh.xcd_sched = fh.sched ? 1u : 0u;
            if (!sched && cap > 0 && gsx::blend_uses_schedule(p.grid, p.semantics, p.generic, n, p.schedule)) {
                if (p.semantics == GSX_SEM_REF_CPU && gsx::knob("GSX_COLD_XCD_SCHED", 1) != 0) {
                    // no schedule on file (a view's first frame, a caller without a hints buffer): the same per-XCD schedule
                    // from THIS frame's list lengths, into the hints buffer's region when there is one (its header then says so)
                    uint32_t *hdr = bh.header ? bh.header : (uint32_t *)(ws + c.sched_header);
                    uint32_t *region = (bh.header && fh.sched_region) ? fh.sched_region : (uint32_t *)(ws + c.sched);
                    if (!(bh.header && !fh.sched_region)) {
                        GSX_HIP(gsx::launch_tile_schedule_xcd(ranges, p.grid.count(), p.grid.nwy(), region, hdr, s));
                        sched = region;
                        bh.header = hdr;
                        bh.xcd_sched = 1u;
                    }
                }
                if (!sched) {       // (the other rule sets: one workgroup ranks the whole frame)
                    sched = (uint32_t *)(ws + c.sched);
                    GSX_HIP(gsx::launch_tile_schedule(ranges, p.grid.count(), (uint32_t *)(ws + c.sched), s));
                }
            }
            tm.mark();  // 4: tile sort (+ the compositing schedule)
            bh.plain = p.plain ? 1u : 0u;
            redo_counted = p.semantics == GSX_SEM_REF_CPU && p.grid.tile == 16 && !p.generic;
            // The 128 spare workgroups hold 16 wave slots of every XCD for ~15 us.  In front of the tiles that is free
            // -- unless the window's tiles fill the chip's 8 192 wave slots just about once (1080p: 7 973 tiles): then
            // some tiles find no slot until the spare workgroups are done.  Behind the tiles they are dispatched as
            // slots free up -- late, so only a frame whose compositing lasts several times their 15 us takes them
            // there (pairs per tile, from the pair capacity = last frame's count).  Measured under rocprofv3, same box:
            // uniform 1M / 1080p 239 us either way, heavy-tailed 1M / 1080p 382 -> 368 us; a 100k frame (36 us of
            // compositing) loses 10 us with them last.
            const int64_t ntl = p.grid.count();
            bh.rank_last = (fh.sched && ntl > 7400 && ntl <= 8192 && (int64_t)cap >= 128 * ntl) ? 1u : 0u;
            if (gsx::knob("GSX_RANK_LAST", -1) >= 0) bh.rank_last = (uint32_t)gsx::knob("GSX_RANK_LAST", -1);   // test library only
            if (p.n_parts > 1 && gsx::blend_in_parts(p.grid, p.semantics, p.generic)) {
                // GsxParams.n_substrips: the same launch once per part of the window, an event of the caller's behind each
                // (a part without tiles is not launched; its event still marks "everything before it is done")
                bool first = true;
                for (int k = 0; k < p.n_parts; ++k) {
                    const gsx::TileSpan span{p.part_axis, p.part_bounds[k], p.part_bounds[k + 1], first ? 1u : 0u, (uint32_t)k};
                    if (span.hi > span.lo || (first && k == p.n_parts - 1)) {
                        GSX_HIP(gsx::launch_blend((const gsx::Record *)(ws + c.rec), (const float4 *)(ws + c.bbox), sorted_vals,
                                                  ranges, p.grid, p.out, p.semantics, p.background, p.generic,
                                                  make_clear_plan(p, false), lt, sched, bh, s, &span));
                        first = false;
                    }
                    GSX_HIP(hipEventRecord((hipEvent_t)p.part_events[k], s));
                }
                parts_marked = true;
            } else {
                GSX_HIP(gsx::launch_blend((const gsx::Record *)(ws + c.rec), (const float4 *)(ws + c.bbox), sorted_vals,
                                          ranges, p.grid, p.out, p.semantics, p.background, p.generic,
                                          make_clear_plan(p, false), lt, sched, bh, s));
            }
            tm.mark();  // 5: blend
        }
    }
    if (!parts_marked)
        for (int k = 0; k < p.n_parts; ++k) GSX_HIP(hipEventRecord((hipEvent_t)p.part_events[k], s));
    if (p.no_sync) {
        if (stats) {
            // stats must be pinned host memory; the two counts land when the stream gets here
            if (!counts_on_device) {
                stats->n_visible = 0;
                stats->n_instances = 0;
                stats->n_kept = 0;
            } else if (!counts_in_host) {
                GSX_HIP(hipMemcpyAsync(stats, dev2, 16, hipMemcpyDeviceToHost, s));
                GSX_HIP(hipMemcpyAsync(&stats->n_kept, dev2 + 2, 8, hipMemcpyDeviceToHost, s));
            }
            if (has_redo) {             // GsxParams.stats_size: the caller's struct reaches n_redo
                stats->n_redo = 0;      // (the upper half stays: the device count has 32 bits)
                if (redo_counted) GSX_HIP(hipMemcpyAsync(&stats->n_redo, ws + c.redo, 4, hipMemcpyDeviceToHost, s));
            }
            stats->n_tiles = p.grid.count();
            stats->reserved = cap;  // > 0: counts are delivered asynchronously; value = pair capacity used
        }
        return GSX_OK;
    }
    int64_t host2[3];
    uint32_t redo_host = 0;
    const int rc = read_counts(c, ws, cap, counts_on_device, redo_counted ? &redo_host : nullptr, host2, s);
    if (rc != GSX_OK && rc != GSX_ERR_WORKSPACE_TOO_SMALL) return rc;
    if (stats) {
        stats->n_visible = host2[0];
        stats->n_instances = host2[1];
        stats->n_kept = host2[2];
        if (has_redo) stats->n_redo = redo_host;
        stats->n_tiles = p.grid.count();
        stats->reserved = 0;
    }
    tm.finish(stats);
    return rc;
}

#ifdef GSX_TEST_HOOKS
// test library only (gsx_debug.h: gsx_debug_backward_stage_ms): the last gsx_render_backward call's stages under GSX_FLAG_TIMING
thread_local float g_backward_ms[3] = {0.0f, 0.0f, 0.0f};
#endif

// The three outputs gsx_render_backward_geometry adds, and the two gsx_render_backward_screen adds to those (null / null:
// the geometry entry; radius may be null on its own).
struct GeometryGrads {
    float *means3d, *scales, *quats;
    float *means2d = nullptr, *radius = nullptr;
    float *world2view = nullptr, *full_proj = nullptr;     // gsx_render_backward_camera: both, 16 floats each
    const float *depth = nullptr, *grad_depth = nullptr;   // gsx_render_backward_depth: both, the (D, A) image and dL/d(D, A)
    float *means2d_abs = nullptr;                           // gsx_render_backward_screen_abs: (n,2); excludes the two lines above
};

// ---- The entries that walk the forward's lists again: the gradient entries, gsx_render_depth, gsx_render_contribution.

// The rule sets such an entry accepts: the reference's own frame, the published one, or either.
enum { kRulesRefCpu = 1, kRulesStd3dgs = 2, kRulesEither = kRulesRefCpu | kRulesStd3dgs };

int check_rules(const Plan &p, int rules, const char *entry) {
    if (rules == kRulesRefCpu) {
        if (p.antialiased) return fail(GSX_ERR_INVALID_ARGUMENT, "%s does not take GSX_FLAG_ANTIALIASED: it supports GSX_SEM_REF_CPU only", entry);
        if (p.semantics != GSX_SEM_REF_CPU) return fail(GSX_ERR_INVALID_ARGUMENT, "%s supports GSX_SEM_REF_CPU only", entry);
    } else if (rules == kRulesStd3dgs) {
        if (p.semantics != GSX_SEM_STD_3DGS)
            return fail(GSX_ERR_INVALID_ARGUMENT, "%s: params->semantics must be GSX_SEM_STD_3DGS", entry);
    } else if (p.semantics == GSX_SEM_REF_CUDA) {
        return fail(GSX_ERR_INVALID_ARGUMENT, "%s: GSX_SEM_REF_CUDA is not supported (GSX_SEM_REF_CPU or GSX_SEM_STD_3DGS)", entry);
    }
    return GSX_OK;
}

// The arguments all these entries share.
struct WalkArgs {
    const GsxCamera *camera;
    const float *means3d, *scales, *quats, *opacity_logit, *colors;
    int64_t n;
    int32_t tile_size;
    const GsxParams *params;
    void *workspace;
    size_t workspace_bytes;
    void *stream;
};

// What the opening leaves: open_walk fills the first line, lists_again the second, launch_walk_prefix the third.
struct Walk {
    Plan p; Carve c; int64_t cap; char *ws; hipStream_t s;
    gsx::GaussiansIn in; const uint32_t *order, *sorted_vals; const gsx::TileRect *rrect; uint32_t m; int64_t counts[3];
    uint32_t *prefix, *rank_of; float4 *slots, *geo_slots;
};

// Validation, up to and including the workspace (a.camera is not NULL: the entry has said so, and whatever else it
// says before there is a plan).  frame: the array the plan describes; rules: kRules*; outputs_fault: the entry's
// complaint about its output arrays, or null -- it speaks here, between the inputs and the workspace; mode: kCarve*.
int open_walk(const WalkArgs &a, const char *entry, int rules, float *frame, const char *outputs_fault, int mode, Walk &w) {
    const int32_t width = a.camera->width, height = a.camera->height;
    int rc = make_plan_or_fail(width, height, a.tile_size, frame, a.params, w.p);
    if (rc != GSX_OK) return rc;
    rc = check_rules(w.p, rules, entry);
    if (rc != GSX_OK) return rc;
    char msg[256];
    rc = check_whole_frame(w.p, width, height, a.params, entry, msg, sizeof msg);
    if (rc != GSX_OK) return fail(rc, "%s", msg);
    rc = check_inputs(w.p, a.n, a.means3d, a.scales, a.quats, a.opacity_logit, a.colors);
    if (rc != GSX_OK) return rc;
    if (outputs_fault) return fail(GSX_ERR_INVALID_ARGUMENT, "%s", outputs_fault);
    rc = check_workspace(a.workspace, a.workspace_bytes, a.n, max_tiles_of(width, height, a.tile_size), w.c, w.cap, mode);
    if (rc != GSX_OK) return rc;
    w.ws = (char *)a.workspace;
    w.s = (hipStream_t)a.stream;
    return GSX_OK;
}

// An entry's outputs, zeroed in the order given: rows no tile lists, and frames that list nothing, read zero.
struct ZeroFill {
    void *ptr;      // null: not asked for, skipped
    size_t words;
};
int zero_fill(std::initializer_list<ZeroFill> outputs, hipStream_t s) {
    for (const ZeroFill &z : outputs)
        if (z.ptr) GSX_HIP(gsx::launch_zero_words((uint32_t *)z.ptr, z.words, s));
    return GSX_OK;
}

// Behind the entry's zero-fill.  Without a Gaussian or a tile the stream is synchronised and nothing more is done;
// otherwise the forward's chain on the same inputs, without the hints buffer: projection, depth order, pairs, tile sort
// and the count read-back, which synchronises (tm: nullptr = no mark behind it).  That leaves in, order, rrect,
// sorted_vals, counts = (n_visible, D, M) and m.  go: the frame lists something, there are pairs to walk -- false with
// GSX_OK: the outputs stand as they were zero-filled.
int lists_again(const WalkArgs &a, Walk &w, StageTimer *tm, bool &go) {
    go = false;
    if (a.n == 0 || w.p.grid.count() == 0) {
        GSX_HIP(hipStreamSynchronize(w.s));
        return GSX_OK;
    }
    w.in = gsx::GaussiansIn{a.means3d, a.scales, a.quats, a.opacity_logit, a.colors, w.p.original_index, nullptr};
    w.rrect = (const gsx::TileRect *)(w.ws + w.c.rrect);
    bool sampled;
    int rc = project_and_sort(w.p, w.c, w.ws, *a.camera, w.in, a.n, w.cap, nullptr, nullptr, w.s, w.order, sampled);
    if (rc == GSX_OK) {
        uint32_t *counters = (uint32_t *)(w.ws + w.c.counters);
        const gsx::BinCounts bcnt{(int64_t *)(counters + 4), nullptr, counters + kCtrPairs, counters + kCtrLong,
                                  (uint32_t *)(w.ws + w.c.redo), counters + kCtrCulled, a.n};
        const gsx::LongTiles lt{counters + kCtrLong, (uint32_t *)(w.ws + w.c.longs), 0u};     // no long-tile split: plain [first, last)
        w.sorted_vals = nullptr;
        rc = bin_pairs(w.p, w.c, w.ws, a.n, w.cap, w.rrect, w.order, counters + kCtrKept, sampled, bcnt, lt, nullptr, w.s, w.sorted_vals);
    }
    if (rc == GSX_OK) rc = read_counts(w.c, w.ws, w.cap, true, nullptr, w.counts, w.s);
    if (tm) tm->mark();
    if (rc != GSX_OK) return rc;
    w.m = (uint32_t)w.counts[2];
    go = w.m != 0 && w.counts[1] != 0;
    return GSX_OK;
}

// For the bodies that leave sums per pair: every rank's first slot and every row's rank (launch_backward_prefix), and
// where the slots are (geo: the second slot array of kCarveGeometry and up as well).
int launch_walk_prefix(Walk &w, bool geo) {
    w.prefix = (uint32_t *)(w.ws + w.c.prefix);
    w.rank_of = (uint32_t *)(w.ws + w.c.rank_of);
    w.slots = (float4 *)(w.ws + w.c.slots);
    w.geo_slots = geo ? (float4 *)(w.ws + w.c.geo_slots) : nullptr;
    GSX_HIP(gsx::launch_backward_prefix(w.rrect, w.order, w.m, w.prefix, w.rank_of, (uint32_t *)(w.ws + w.c.bsum), w.s));
    return GSX_OK;
}
// ... and what the per-Gaussian launches behind the tile kernels take of it
gsx::RankSlots rank_slots(const Walk &w) { return gsx::RankSlots{w.slots, w.geo_slots, w.prefix, w.order, w.m}; }

// What gsx_render_backward and gsx_render_backward_std say about a missing one of the three
const char *const kNoGradArrays = "grad_image / grad_colors / grad_opacity_logit is NULL";

// gsx_render_backward (geo == nullptr) and gsx_render_backward_geometry: one body.  The geometry call carves the third
// workspace mode, runs the tile kernel's geometry instance and, after the colour sums, the per-Gaussian chain.
int render_backward(const WalkArgs &a, const float *image, const float *grad_image, float *grad_colors,
                    float *grad_opacity_logit, const GeometryGrads *geo) {
    if (!a.camera) return fail(GSX_ERR_INVALID_ARGUMENT, "camera is NULL");
    Walk w;
    int rc = open_walk(a, "gsx_render_backward", kRulesRefCpu, const_cast<float *>(image),
                       !grad_image || !grad_colors || !grad_opacity_logit ? kNoGradArrays : nullptr,
                       geo ? (geo->depth ? kCarveDepth : (geo->world2view ? kCarveCamera : kCarveGeometry)) : kCarveBackward, w);
    if (rc != GSX_OK) return rc;
    const Plan &p = w.p;
    const int64_t n = a.n;
    hipStream_t s = w.s;
    StageTimer tm;
    tm.begin(p.timing, s);
    const GeometryGrads g = geo ? *geo : GeometryGrads{nullptr, nullptr, nullptr};
    rc = zero_fill({{grad_colors, (size_t)n * 3}, {grad_opacity_logit, (size_t)n}, {g.means3d, (size_t)n * 3},
                    {g.scales, (size_t)n * 3}, {g.quats, (size_t)n * 4}, {g.means2d, (size_t)n * 2}, {g.radius, (size_t)n},
                    {g.means2d_abs, (size_t)n * 2}, {g.world2view, 16}, {g.full_proj, 16}}, s);   // (the two matrices: 32 exact +0)
    if (rc != GSX_OK) return rc;
    bool go;
    rc = lists_again(a, w, &tm, go);     // mark 1: the forward's stages
    if (rc != GSX_OK || !go) return rc;
    // ---- the backward kernels
    gsx::Record *raw = (gsx::Record *)(w.ws + w.c.raw);
    GSX_HIP(gsx::launch_project_raw(*a.camera, w.in, n, p.small_batch, raw, s));
    rc = launch_walk_prefix(w, geo != nullptr);
    if (rc != GSX_OK) return rc;
    const gsx::BackwardTiles bt{raw, w.sorted_vals, (const uint2 *)(w.ws + w.c.ranges), w.rank_of, w.prefix, w.rrect, image,
                                grad_image, w.slots, w.geo_slots};
    if (geo && geo->depth) {
        float *zrow = (float *)(w.ws + w.c.zrow);
        GSX_HIP(gsx::launch_project_depth(*a.camera, a.means3d, n, p.small_batch, zrow, s));
        GSX_HIP(gsx::launch_backward_tiles_depth(bt, gsx::DepthTiles{zrow, geo->depth, geo->grad_depth}, p.grid, p.out, s));
    } else if (geo && geo->means2d_abs) {
        GSX_HIP(gsx::launch_backward_tiles_abs(bt, p.grid, p.out, s));
    } else {
        GSX_HIP(gsx::launch_backward_tiles(bt, p.grid, p.out, s));
    }
    tm.mark();  // 2: raw records, prefix, compositing backward
    const gsx::RankSlots rk = rank_slots(w);
    GSX_HIP(gsx::launch_backward_sums(rk, raw, grad_colors, grad_opacity_logit, s));
    const gsx::GeometryRows rows{a.means3d, a.scales, a.quats, g.means3d, g.scales, g.quats, g.means2d,
                                 g.means2d ? g.radius : nullptr};
    if (geo && geo->depth) {
        GSX_HIP(gsx::launch_backward_geometry_depth(*a.camera, rk, raw, rows, s));
    } else if (geo) {
        const gsx::CameraGrads cg{geo->world2view, geo->full_proj, (float *)(w.ws + w.c.cam_partials)};
        GSX_HIP(gsx::launch_backward_geometry(*a.camera, rk, raw, rows, s, geo->world2view ? &cg : nullptr, geo->means2d_abs));
    }
    tm.mark();  // 3: sums (and the geometry chain)
    GSX_HIP(hipStreamSynchronize(s));
#ifdef GSX_TEST_HOOKS
    if (p.timing) {
        GsxFrameStats st;
        memset(&st, 0, sizeof st);
        tm.finish(&st);
        for (int i = 0; i < 3; ++i) g_backward_ms[i] = st.stage_ms[i];
    }
#endif
    return GSX_OK;
}

}  // namespace

extern "C" {

int gsx_version(void) { return GSX_VERSION; }

const char *gsx_last_error(void) { return g_error; }

void gsx_default_params_sized(GsxParams *params, size_t struct_size) {
    if (params) default_params(params, struct_size);
}

// the symbol binaries built against the ABI 300 / 301 headers call (there a plain function, the struct 104 bytes):
// the name is parenthesised because this header makes it a macro
void (gsx_default_params)(GsxParams *params) {
    if (params) default_params(params, kParamsBytesAbi300);
}

size_t gsx_hints_bytes(int32_t width, int32_t height, int32_t tile) {
    if (width <= 0 || height <= 0 || tile <= 0) return 0;
    return gsx::hints_layout(max_tiles_of(width, height, tile), max_axis_tiles_of(width, height, tile)).total;
}

size_t gsx_workspace_bytes(int64_t n, int32_t width, int32_t height, int32_t tile, int64_t max_instances) {
    return workspace_bytes(n, width, height, tile, max_instances, kCarveForward);
}

int gsx_preprocess(const GsxCamera *camera, const float *means3d, const float *scales, const float *quats,
                   const float *opacity_logit, const float *colors, int64_t n, float *points_xy, float *colors_out,
                   float *covariance_2d, float *depths, float *inverse_covariance_2d, float *radius, float *min_x,
                   float *max_x, float *min_y, float *max_y, float *sigmoid_opacity, int32_t *order,
                   int64_t *n_visible_host, const GsxParams *params, void *workspace, size_t workspace_bytes,
                   void *stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!camera) return fail(GSX_ERR_INVALID_ARGUMENT, "camera is NULL");
    if (n < 0 || n >= (int64_t)1 << 31) return fail(GSX_ERR_INVALID_ARGUMENT, "n = %lld out of range", (long long)n);
    if (params && (params->flags & GSX_FLAG_ANTIALIASED))
        return fail(GSX_ERR_INVALID_ARGUMENT, "gsx_preprocess does not take GSX_FLAG_ANTIALIASED: it is the reference's stage 1, not GSX_SEM_STD_3DGS's");
    const int small_batch = !params ? 0 : ((params->flags & GSX_FLAG_ONE_VISIBLE) ? 1 : ((params->flags & GSX_FLAG_SMALL_BATCH) ? 2 : 0));
    if (n_visible_host) *n_visible_host = 0;
    if (n == 0) return GSX_OK;
    if (!means3d || !scales || !quats || !opacity_logit || !colors) return fail(GSX_ERR_INVALID_ARGUMENT, "an input array is NULL");
    if (!points_xy || !colors_out || !covariance_2d || !depths || !inverse_covariance_2d || !radius || !min_x || !max_x ||
        !min_y || !max_y || !sigmoid_opacity)
        return fail(GSX_ERR_INVALID_ARGUMENT, "an output array is NULL");
    Carve c;
    int64_t cap;
    int rc = check_workspace(workspace, workspace_bytes, n, 1, c, cap);
    if (rc != GSX_OK) return rc;
    char *ws = (char *)workspace;
    uint32_t *k0 = (uint32_t *)(ws + c.keys0), *k1 = (uint32_t *)(ws + c.keys1);
    uint32_t *v0 = (uint32_t *)(ws + c.vals0), *v1 = (uint32_t *)(ws + c.vals1);
    uint32_t *counters = (uint32_t *)(ws + c.counters);
    // Three steps.  (1) Original order, coalesced: depth key + the projected quantities of every visible Gaussian in
    // its record slot (the kernel also zeroes the sort's counters).  (2) The SAME compacting depth sort as the
    // whole-path entry: it drops -- and counts -- the culled Gaussians in its first step and leaves the index of every
    // depth rank (the rectangles it carries along are not needed here: it moves whatever the workspace holds).
    // (3) Rank order: one 48-byte gather per rank, the derived fields, eleven coalesced output arrays.  Round 2 ran a
    // memset node, a key kernel, a 12-launch LSD sort over all n keys, a counting kernel and a projection that
    // gathered the five input arrays by rank.
    gsx::GaussiansIn in{means3d, scales, quats, opacity_logit, colors, original_index_of(params)};
    gsx::Record *stage = (gsx::Record *)(ws + c.rec);
    GSX_HIP(gsx::launch_project_stage(*camera, in, n, k0, stage, counters, small_batch, s));
    const gsx::DepthRoute route = gsx::depth_sort_route(n, 0);
    if (route != gsx::kDepthLsd)
        GSX_HIP(gsx::sort_depth_sampled(route, ws + c.temp, k0, k1, v0, v1, n, 0, counters + kCtrKept, counters + kCtrCulled,
                                        (const gsx::TileRect *)(ws + c.rect), (gsx::TileRect *)(ws + c.rrect), 0, nullptr,
                                        gsx::SortHints{nullptr, nullptr, nullptr, false}, s));
    else
        GSX_HIP(gsx::sort_depth_compact(ws + c.temp, k0, k1, v0, v1, n, counters + kCtrKept, counters + kCtrCulled,
                                        (const gsx::TileRect *)(ws + c.rect), (gsx::TileRect *)(ws + c.rrect), s));
    gsx::StageOneOut out{points_xy, colors_out, covariance_2d, depths, inverse_covariance_2d, radius,
                         min_x, max_x, min_y, max_y, sigmoid_opacity, order};
    GSX_HIP(gsx::launch_project_full(stage, v0, counters + kCtrKept, n, out, s));
    uint32_t nv = 0;
    GSX_HIP(hipMemcpyAsync(&nv, counters + kCtrKept, 4, hipMemcpyDeviceToHost, s));
    GSX_HIP(hipStreamSynchronize(s));
    if (n_visible_host) *n_visible_host = nv;
    return GSX_OK;
}

int gsx_render_preprocessed(int32_t image_height, int32_t image_width, int32_t tile_size, const float *point_means,
                            const float *point_colors, const float *inverse_covariance_2d, const float *min_x,
                            const float *max_x, const float *min_y, const float *max_y, const float *opacity,
                            int64_t n, float *out_image, const GsxParams *params, GsxFrameStats *stats_host,
                            void *workspace, size_t workspace_bytes, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    Plan p;
    int rc = make_plan_or_fail(image_width, image_height, tile_size, out_image, params, p);
    if (rc != GSX_OK) return rc;
    if (p.antialiased)
        return fail(GSX_ERR_INVALID_ARGUMENT, "gsx_render_preprocessed does not take GSX_FLAG_ANTIALIASED: GSX_SEM_STD_3DGS has its own stage 1, use gsx_render_forward");
    if (p.semantics == GSX_SEM_STD_3DGS)
        return fail(GSX_ERR_UNSUPPORTED, "GSX_SEM_STD_3DGS has its own stage 1: use gsx_render_forward");
    if (n < 0 || n >= (int64_t)1 << 31) return fail(GSX_ERR_INVALID_ARGUMENT, "n = %lld out of range", (long long)n);
    if (n > 0 && (!point_means || !point_colors || !inverse_covariance_2d || !min_x || !max_x || !min_y || !max_y || !opacity))
        return fail(GSX_ERR_INVALID_ARGUMENT, "an input array is NULL");
    Carve c;
    int64_t cap;
    rc = check_workspace(workspace, workspace_bytes, n, max_tiles_of(image_width, image_height, tile_size), c, cap);
    if (rc != GSX_OK) return rc;
    char *ws = (char *)workspace;
    StageTimer tm;
    tm.begin(p.timing, s);
    tm.mark();  // 1: (no depth sort on this entry point)
    gsx::PreprocessedIn in{point_means, point_colors, inverse_covariance_2d, min_x, max_x, min_y, max_y, opacity};
    GSX_HIP(gsx::launch_pack_preprocessed(in, n, p.grid, p.semantics, (gsx::Record *)(ws + c.rec),
                                          (gsx::TileRect *)(ws + c.rect),
                                          p.semantics != GSX_SEM_STD_3DGS ? (float4 *)(ws + c.bbox) : nullptr, s));
    tm.mark();  // 2: pack
    // rows are already in compositing order: the rectangles by row ARE the rectangles by rank
    return bin_and_blend(p, c, ws, n, cap, (const gsx::TileRect *)(ws + c.rect), nullptr, nullptr, nullptr, false, stats_host,
                         tm, s);
}

int gsx_render_forward(const GsxCamera *camera, const float *means3d, const float *scales, const float *quats,
                       const float *opacity_logit, const float *colors, int64_t n, int32_t tile_size,
                       float *out_image, const GsxParams *params, GsxFrameStats *stats_host, void *workspace,
                       size_t workspace_bytes, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!camera) return fail(GSX_ERR_INVALID_ARGUMENT, "camera is NULL");
    Plan p;
    int rc = make_plan_or_fail(camera->width, camera->height, tile_size, out_image, params, p);
    if (rc != GSX_OK) return rc;
    rc = check_inputs(p, n, means3d, scales, quats, opacity_logit, colors);
    if (rc != GSX_OK) return rc;
    if (p.n_parts > 0) {
        // substrip_events are recorded with plain hipEventRecord: inside a stream capture they would become nodes of
        // the graph, and the caller's hipStreamWaitEvent on another stream would fail or invalidate the capture
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        GSX_HIP(hipStreamIsCapturing(s, &cs));
        if (cs != hipStreamCaptureStatusNone)
            return fail(GSX_ERR_UNSUPPORTED, "n_substrips cannot be combined with stream capture (the part events are recorded on the stream)");
    }
    Carve c;
    int64_t cap;
    rc = check_workspace(workspace, workspace_bytes, n, max_tiles_of(camera->width, camera->height, tile_size), c, cap);
    if (rc != GSX_OK) return rc;
    char *ws = (char *)workspace;
    StageTimer tm;
    tm.begin(p.timing, s);
    const gsx::GaussiansIn in{means3d, scales, quats, opacity_logit, p.sh ? p.sh : colors, p.original_index, (const float4 *)p.block_bounds};
    FrameHints fh;
    const uint32_t *order;
    bool sampled;
    rc = project_and_sort(p, c, ws, *camera, in, n, cap, &fh, &tm, s, order, sampled);
    if (rc != GSX_OK) return rc;
    uint32_t *counters = (uint32_t *)(ws + c.counters);
    return bin_and_blend(p, c, ws, n, cap, (const gsx::TileRect *)(ws + c.rrect), order, counters + kCtrKept,
                         counters + kCtrCulled, sampled, stats_host, tm, s, fh);
}

size_t gsx_backward_workspace_bytes(int64_t n, int32_t width, int32_t height, int32_t tile, int64_t max_instances) {
    return workspace_bytes(n, width, height, tile, max_instances, kCarveBackward);
}

size_t gsx_backward_geometry_workspace_bytes(int64_t n, int32_t width, int32_t height, int32_t tile, int64_t max_instances) {
    return workspace_bytes(n, width, height, tile, max_instances, kCarveGeometry);
}

int gsx_render_backward(const GsxCamera *camera, const float *means3d, const float *scales, const float *quats,
                        const float *opacity_logit, const float *colors, int64_t n, int32_t tile_size,
                        const float *image, const float *grad_image, float *grad_colors, float *grad_opacity_logit,
                        const GsxParams *params, void *workspace, size_t workspace_bytes, void *stream) {
    const WalkArgs a{camera, means3d, scales, quats, opacity_logit, colors, n, tile_size, params, workspace, workspace_bytes, stream};
    return render_backward(a, image, grad_image, grad_colors, grad_opacity_logit, nullptr);
}

int gsx_render_backward_geometry(const GsxCamera *camera, const float *means3d, const float *scales, const float *quats,
                                 const float *opacity_logit, const float *colors, int64_t n, int32_t tile_size,
                                 const float *image, const float *grad_image, float *grad_colors, float *grad_opacity_logit,
                                 float *grad_means3d, float *grad_scales, float *grad_quats, const GsxParams *params,
                                 void *workspace, size_t workspace_bytes, void *stream) {
    if (!grad_means3d || !grad_scales || !grad_quats)
        return fail(GSX_ERR_INVALID_ARGUMENT, "grad_means3d / grad_scales / grad_quats is NULL");
    const GeometryGrads geo{grad_means3d, grad_scales, grad_quats};
    const WalkArgs a{camera, means3d, scales, quats, opacity_logit, colors, n, tile_size, params, workspace, workspace_bytes, stream};
    return render_backward(a, image, grad_image, grad_colors, grad_opacity_logit, &geo);
}

int gsx_render_backward_screen(const GsxCamera *camera, const float *means3d, const float *scales, const float *quats,
                               const float *opacity_logit, const float *colors, int64_t n, int32_t tile_size,
                               const float *image, const float *grad_image, float *grad_colors, float *grad_opacity_logit,
                               float *grad_means3d, float *grad_scales, float *grad_quats, float *grad_means2d,
                               float *screen_radius, const GsxParams *params, void *workspace, size_t workspace_bytes,
                               void *stream) {
    if (!grad_means3d || !grad_scales || !grad_quats)
        return fail(GSX_ERR_INVALID_ARGUMENT, "grad_means3d / grad_scales / grad_quats is NULL");
    if (!grad_means2d) return fail(GSX_ERR_INVALID_ARGUMENT, "grad_means2d is NULL");
    const GeometryGrads geo{grad_means3d, grad_scales, grad_quats, grad_means2d, screen_radius};
    const WalkArgs a{camera, means3d, scales, quats, opacity_logit, colors, n, tile_size, params, workspace, workspace_bytes, stream};
    return render_backward(a, image, grad_image, grad_colors, grad_opacity_logit, &geo);
}

int gsx_render_backward_screen_abs(const GsxCamera *camera, const float *means3d, const float *scales, const float *quats,
                                   const float *opacity_logit, const float *colors, int64_t n, int32_t tile_size,
                                   const float *image, const float *grad_image, float *grad_colors, float *grad_opacity_logit,
                                   float *grad_means3d, float *grad_scales, float *grad_quats, float *grad_means2d,
                                   float *screen_radius, float *grad_means2d_abs, const GsxParams *params, void *workspace,
                                   size_t workspace_bytes, void *stream) {
    if (!grad_means3d || !grad_scales || !grad_quats)
        return fail(GSX_ERR_INVALID_ARGUMENT, "grad_means3d / grad_scales / grad_quats is NULL");
    if (!grad_means2d) return fail(GSX_ERR_INVALID_ARGUMENT, "grad_means2d is NULL");
    if (!screen_radius) return fail(GSX_ERR_INVALID_ARGUMENT, "screen_radius is NULL");
    if (!grad_means2d_abs) return fail(GSX_ERR_INVALID_ARGUMENT, "grad_means2d_abs is NULL");
    GeometryGrads geo{grad_means3d, grad_scales, grad_quats, grad_means2d, screen_radius};
    geo.means2d_abs = grad_means2d_abs;
    const WalkArgs a{camera, means3d, scales, quats, opacity_logit, colors, n, tile_size, params, workspace, workspace_bytes, stream};
    return render_backward(a, image, grad_image, grad_colors, grad_opacity_logit, &geo);
}

size_t gsx_backward_std_workspace_bytes(int64_t n, int32_t width, int32_t height, int32_t tile, int64_t max_instances) {
    return workspace_bytes(n, width, height, tile, max_instances, kCarveGeometry);
}

// gsx_render_backward_std: render_backward's order of work on the GSX_SEM_STD_3DGS frame.  The forward's chain leaves the
// packed records the std tile kernels read (no raw projection); the workspace is the geometry entry's.
int gsx_render_backward_std(const GsxCamera *camera, const float *means3d, const float *scales, const float *quats,
                            const float *opacity_logit, const float *colors, int64_t n, int32_t tile_size,
                            const float *image, const float *grad_image, float *grad_colors, float *grad_opacity_logit,
                            float *grad_means3d, float *grad_scales, float *grad_quats, float *grad_means2d,
                            float *screen_radius, const GsxParams *params, void *workspace, size_t workspace_bytes,
                            void *stream) {
    const char *entry = "gsx_render_backward_std";
    if (!camera) return fail(GSX_ERR_INVALID_ARGUMENT, "camera is NULL");
    if (!params) return fail(GSX_ERR_INVALID_ARGUMENT, "params is NULL: %s needs params->semantics = GSX_SEM_STD_3DGS", entry);
    if (!image) return fail(GSX_ERR_INVALID_ARGUMENT, "image is NULL");
    const int n_geo = (grad_means3d != nullptr) + (grad_scales != nullptr) + (grad_quats != nullptr);
    const bool geo = n_geo == 3;
    const char *outputs_fault = nullptr;
    if (!grad_image || !grad_colors || !grad_opacity_logit)
        outputs_fault = kNoGradArrays;
    else if (n_geo != 0 && n_geo != 3)
        outputs_fault = "grad_means3d / grad_scales / grad_quats: all three or none";
    else if ((grad_means2d != nullptr) != (screen_radius != nullptr))
        outputs_fault = "grad_means2d / screen_radius: both or none";
    else if (grad_means2d && !geo)
        outputs_fault = "grad_means2d and screen_radius need grad_means3d, grad_scales and grad_quats";
    const WalkArgs a{camera, means3d, scales, quats, opacity_logit, colors, n, tile_size, params, workspace, workspace_bytes, stream};
    Walk w;
    int rc = open_walk(a, entry, kRulesStd3dgs, const_cast<float *>(image), outputs_fault, kCarveGeometry, w);
    if (rc != GSX_OK) return rc;
    hipStream_t s = w.s;
    // (the three, and the two, are all there or all NULL)
    rc = zero_fill({{grad_colors, (size_t)n * 3}, {grad_opacity_logit, (size_t)n}, {grad_means3d, (size_t)n * 3},
                    {grad_scales, (size_t)n * 3}, {grad_quats, (size_t)n * 4}, {grad_means2d, (size_t)n * 2},
                    {screen_radius, (size_t)n}}, s);
    if (rc != GSX_OK) return rc;
    bool go;
    rc = lists_again(a, w, nullptr, go);
    if (rc != GSX_OK || !go) return rc;
    const gsx::Record *rec = (const gsx::Record *)(w.ws + w.c.rec);
    rc = launch_walk_prefix(w, geo);
    if (rc != GSX_OK) return rc;
    const gsx::BackwardTiles bt{rec, w.sorted_vals, (const uint2 *)(w.ws + w.c.ranges), w.rank_of, w.prefix, w.rrect, image,
                                grad_image, w.slots, w.geo_slots};
    GSX_HIP(gsx::launch_backward_tiles_std(bt, w.p.grid, w.p.out, s));
    const gsx::RankSlots rk = rank_slots(w);
    const gsx::GeometryRows rows{means3d, scales, quats, grad_means3d, grad_scales, grad_quats, grad_means2d, screen_radius};
    if (w.p.antialiased) {
        GSX_HIP(gsx::launch_backward_std_antialiased(*camera, rk, rows, opacity_logit, grad_colors, grad_opacity_logit, s));
    } else {
        GSX_HIP(gsx::launch_backward_sums_std(rk, rec, grad_colors, grad_opacity_logit, s));
        if (geo) GSX_HIP(gsx::launch_backward_geometry_std(*camera, rk, rows, s));
    }
    GSX_HIP(hipStreamSynchronize(s));
    return GSX_OK;
}

size_t gsx_contribution_workspace_bytes(int64_t n, int32_t width, int32_t height, int32_t tile, int64_t max_instances) {
    return workspace_bytes(n, width, height, tile, max_instances, kCarveBackward);
}

// gsx_render_contribution: the gradient entries' chain (lists_again) and walk on either rule set, with no frame and no
// gradient: per row the largest T alpha, their sum and the pixel count (gsx_contribution.hip).  The workspace is
// gsx_render_backward's.
int gsx_render_contribution(const GsxCamera *camera, const float *means3d, const float *scales, const float *quats,
                            const float *opacity_logit, const float *colors, int64_t n, int32_t tile_size, float *weight_max,
                            float *weight_sum, uint32_t *pixels, uint32_t *views, int32_t accumulate, const GsxParams *params,
                            void *workspace, size_t workspace_bytes, void *stream) {
    if (!camera) return fail(GSX_ERR_INVALID_ARGUMENT, "camera is NULL");
    if (!weight_max || !weight_sum || !pixels) return fail(GSX_ERR_INVALID_ARGUMENT, "weight_max / weight_sum / pixels is NULL");
    if (accumulate != 0 && accumulate != 1) return fail(GSX_ERR_INVALID_ARGUMENT, "accumulate = %d is neither 0 nor 1", accumulate);
    const WalkArgs a{camera, means3d, scales, quats, opacity_logit, colors, n, tile_size, params, workspace, workspace_bytes, stream};
    Walk w;
    // (weight_max stands in for the frame the plan describes: this entry has none and writes no pixel)
    int rc = open_walk(a, "gsx_render_contribution", kRulesEither, weight_max, nullptr, kCarveBackward, w);
    if (rc != GSX_OK) return rc;
    hipStream_t s = w.s;
    const bool std_rules = w.p.semantics == GSX_SEM_STD_3DGS;
    if (!accumulate) {      // every row: a Gaussian on no tile list reads +0 / 0
        rc = zero_fill({{weight_max, (size_t)n}, {weight_sum, (size_t)n}, {pixels, (size_t)n}, {views, (size_t)n}}, s);
        if (rc != GSX_OK) return rc;
    }
    bool go;
    rc = lists_again(a, w, nullptr, go);
    if (rc != GSX_OK || !go) return rc;
    gsx::Record *raw = (gsx::Record *)(w.ws + w.c.raw);
    if (!std_rules) GSX_HIP(gsx::launch_project_raw(*camera, w.in, n, w.p.small_batch, raw, s));
    rc = launch_walk_prefix(w, false);
    if (rc != GSX_OK) return rc;
    const gsx::ContributionTiles ct{std_rules ? (const gsx::Record *)(w.ws + w.c.rec) : raw, w.sorted_vals,
                                    (const uint2 *)(w.ws + w.c.ranges), w.rank_of, w.prefix, w.rrect, w.slots};
    GSX_HIP(gsx::launch_contribution_tiles(ct, w.p.grid, std_rules, s));
    GSX_HIP(gsx::launch_contribution_sums(w.slots, w.prefix, w.order, w.m, weight_max, weight_sum, pixels, views, accumulate != 0, s));
    GSX_HIP(hipStreamSynchronize(s));
    return GSX_OK;
}

size_t gsx_backward_camera_workspace_bytes(int64_t n, int32_t width, int32_t height, int32_t tile, int64_t max_instances) {
    return workspace_bytes(n, width, height, tile, max_instances, kCarveCamera);
}

int gsx_render_backward_camera(const GsxCamera *camera, const float *means3d, const float *scales, const float *quats,
                               const float *opacity_logit, const float *colors, int64_t n, int32_t tile_size,
                               const float *image, const float *grad_image, float *grad_colors, float *grad_opacity_logit,
                               float *grad_means3d, float *grad_scales, float *grad_quats, float *grad_means2d,
                               float *screen_radius, float *grad_world2view, float *grad_full_proj, const GsxParams *params,
                               void *workspace, size_t workspace_bytes, void *stream) {
    if (!grad_means3d || !grad_scales || !grad_quats)
        return fail(GSX_ERR_INVALID_ARGUMENT, "grad_means3d / grad_scales / grad_quats is NULL");
    if (!grad_world2view || !grad_full_proj) return fail(GSX_ERR_INVALID_ARGUMENT, "grad_world2view / grad_full_proj is NULL");
    const GeometryGrads geo{grad_means3d, grad_scales, grad_quats, grad_means2d, screen_radius, grad_world2view, grad_full_proj};
    const WalkArgs a{camera, means3d, scales, quats, opacity_logit, colors, n, tile_size, params, workspace, workspace_bytes, stream};
    return render_backward(a, image, grad_image, grad_colors, grad_opacity_logit, &geo);
}

size_t gsx_depth_workspace_bytes(int64_t n, int32_t width, int32_t height, int32_t tile, int64_t max_instances) {
    return workspace_bytes(n, width, height, tile, max_instances, kCarveDepth);
}

size_t gsx_backward_depth_workspace_bytes(int64_t n, int32_t width, int32_t height, int32_t tile, int64_t max_instances) {
    return workspace_bytes(n, width, height, tile, max_instances, kCarveDepth);
}

int gsx_render_depth(const GsxCamera *camera, const float *means3d, const float *scales, const float *quats,
                     const float *opacity_logit, const float *colors, int64_t n, int32_t tile_size, float *depth_out,
                     const GsxParams *params, void *workspace, size_t workspace_bytes, void *stream) {
    if (!camera) return fail(GSX_ERR_INVALID_ARGUMENT, "camera is NULL");
    if (!depth_out) return fail(GSX_ERR_INVALID_ARGUMENT, "depth_out is NULL");
    const WalkArgs a{camera, means3d, scales, quats, opacity_logit, colors, n, tile_size, params, workspace, workspace_bytes, stream};
    Walk w;
    int rc = open_walk(a, "gsx_render_depth", kRulesRefCpu, depth_out, nullptr, kCarveDepth, w);   // (the frame's descriptor: depth_index)
    if (rc != GSX_OK) return rc;
    hipStream_t s = w.s;
    // every pixel: zeros where the frame has zeros (the unrendered last row and column of tiles, a frame that lists nothing)
    rc = zero_fill({{depth_out, (size_t)camera->width * (size_t)camera->height * 2}}, s);
    if (rc != GSX_OK) return rc;
    bool go;
    rc = lists_again(a, w, nullptr, go);
    if (rc != GSX_OK || !go) return rc;
    gsx::Record *raw = (gsx::Record *)(w.ws + w.c.raw);
    float *zrow = (float *)(w.ws + w.c.zrow);
    GSX_HIP(gsx::launch_project_raw(*camera, w.in, n, w.p.small_batch, raw, s));
    GSX_HIP(gsx::launch_project_depth(*camera, means3d, n, w.p.small_batch, zrow, s));
    GSX_HIP(gsx::launch_depth_tiles(raw, w.sorted_vals, (const uint2 *)(w.ws + w.c.ranges), zrow, w.p.grid, w.p.out, depth_out, s));
    GSX_HIP(hipStreamSynchronize(s));
    return GSX_OK;
}

int gsx_render_backward_depth(const GsxCamera *camera, const float *means3d, const float *scales, const float *quats,
                              const float *opacity_logit, const float *colors, int64_t n, int32_t tile_size,
                              const float *image, const float *grad_image, float *grad_colors, float *grad_opacity_logit,
                              float *grad_means3d, float *grad_scales, float *grad_quats, float *grad_means2d,
                              float *screen_radius, const float *depth, const float *grad_depth, const GsxParams *params,
                              void *workspace, size_t workspace_bytes, void *stream) {
    if (!grad_means3d || !grad_scales || !grad_quats)
        return fail(GSX_ERR_INVALID_ARGUMENT, "grad_means3d / grad_scales / grad_quats is NULL");
    if (!depth || !grad_depth) return fail(GSX_ERR_INVALID_ARGUMENT, "depth / grad_depth is NULL");
    GeometryGrads geo{grad_means3d, grad_scales, grad_quats, grad_means2d, screen_radius};
    geo.depth = depth;
    geo.grad_depth = grad_depth;
    const WalkArgs a{camera, means3d, scales, quats, opacity_logit, colors, n, tile_size, params, workspace, workspace_bytes, stream};
    return render_backward(a, image, grad_image, grad_colors, grad_opacity_logit, &geo);
}

#ifdef GSX_TEST_HOOKS
int gsx_debug_backward_stage_ms(float *out3) {
    if (!out3) return fail(GSX_ERR_INVALID_ARGUMENT, "out3 is NULL");
    for (int i = 0; i < 3; ++i) out3[i] = g_backward_ms[i];
    return GSX_OK;
}
#endif

int gsx_sh_to_rgb(const float *means3d, const float *sh, int32_t degree, int64_t n, const float *camera_center_host,
                  float *colors_out, void *stream) {
    if (degree < 0 || degree > 3) return fail(GSX_ERR_INVALID_ARGUMENT, "SH degree %d outside [0,3]", degree);
    if (n < 0) return fail(GSX_ERR_INVALID_ARGUMENT, "n is negative");
    if (!camera_center_host) return fail(GSX_ERR_INVALID_ARGUMENT, "camera_center_host is NULL");
    if (n > 0 && (!means3d || !sh || !colors_out)) return fail(GSX_ERR_INVALID_ARGUMENT, "an array is NULL");
    GSX_HIP(gsx::launch_sh_to_rgb(means3d, sh, degree, n, camera_center_host, colors_out, (hipStream_t)stream));
    return GSX_OK;
}

int gsx_sh_backward(const float *means3d, const float *sh, int32_t degree, int64_t n, const float *camera_center_host,
                    const float *grad_colors, float *grad_sh, float *grad_means3d, void *stream) {
    if (degree < 0 || degree > 3) return fail(GSX_ERR_INVALID_ARGUMENT, "SH degree %d outside [0,3]", degree);
    if (n < 0) return fail(GSX_ERR_INVALID_ARGUMENT, "n is negative");
    if (!camera_center_host) return fail(GSX_ERR_INVALID_ARGUMENT, "camera_center_host is NULL");
    if (n > 0 && (!means3d || !sh || !grad_colors || !grad_sh)) return fail(GSX_ERR_INVALID_ARGUMENT, "an array is NULL");
    GSX_HIP(gsx::launch_sh_backward(means3d, sh, degree, n, camera_center_host, grad_colors, grad_sh, grad_means3d,
                                    (hipStream_t)stream));
    return GSX_OK;
}

// stored_degree / active_degree of the two _active entries: 0 when both are in range, else the failure already filed
static int check_sh_degrees(int32_t stored_degree, int32_t active_degree) {
    if (stored_degree < 0 || stored_degree > 3)
        return fail(GSX_ERR_INVALID_ARGUMENT, "stored_degree %d outside [0,3]", stored_degree);
    if (active_degree < 0 || active_degree > 3)
        return fail(GSX_ERR_INVALID_ARGUMENT, "active_degree %d outside [0,3]", active_degree);
    if (active_degree > stored_degree)
        return fail(GSX_ERR_INVALID_ARGUMENT, "active_degree %d above stored_degree %d", active_degree, stored_degree);
    return GSX_OK;
}

int gsx_sh_to_rgb_active(const float *means3d, const float *sh, int32_t stored_degree, int32_t active_degree, int64_t n,
                         const float *camera_center_host, float *colors_out, void *stream) {
    if (int rc = check_sh_degrees(stored_degree, active_degree)) return rc;
    if (n < 0) return fail(GSX_ERR_INVALID_ARGUMENT, "n is negative");
    if (!camera_center_host) return fail(GSX_ERR_INVALID_ARGUMENT, "camera_center_host is NULL");
    if (n > 0 && (!means3d || !sh || !colors_out)) return fail(GSX_ERR_INVALID_ARGUMENT, "an array is NULL");
    GSX_HIP(gsx::launch_sh_to_rgb_active(means3d, sh, stored_degree, active_degree, n, camera_center_host, colors_out,
                                         (hipStream_t)stream));
    return GSX_OK;
}

int gsx_sh_backward_active(const float *means3d, const float *sh, int32_t stored_degree, int32_t active_degree, int64_t n,
                           const float *camera_center_host, const float *grad_colors, float *grad_sh, float *grad_means3d,
                           void *stream) {
    if (int rc = check_sh_degrees(stored_degree, active_degree)) return rc;
    if (n < 0) return fail(GSX_ERR_INVALID_ARGUMENT, "n is negative");
    if (!camera_center_host) return fail(GSX_ERR_INVALID_ARGUMENT, "camera_center_host is NULL");
    if (n > 0 && (!means3d || !sh || !grad_colors || !grad_sh)) return fail(GSX_ERR_INVALID_ARGUMENT, "an array is NULL");
    GSX_HIP(gsx::launch_sh_backward_active(means3d, sh, stored_degree, active_degree, n, camera_center_host, grad_colors,
                                           grad_sh, grad_means3d, (hipStream_t)stream));
    return GSX_OK;
}

size_t gsx_photometric_loss_workspace_bytes(int32_t rows, int32_t cols, int32_t with_grad) {
    LossCarve c;
    return loss_carve(rows, cols, with_grad != 0, c) ? c.total : 0;
}

// What the two loss entries check alike: the images, the region and the strides, then -- behind whatever else the
// weighted entry says about its arguments -- lambda_dssim.
static int check_loss_images(const gsx::LossImages &im, const float *loss_out) {
    if (!im.image) return fail(GSX_ERR_INVALID_ARGUMENT, "image is NULL");
    if (!im.target) return fail(GSX_ERR_INVALID_ARGUMENT, "target is NULL");
    if (!loss_out) return fail(GSX_ERR_INVALID_ARGUMENT, "loss_out is NULL");
    if (im.rows <= 0) return fail(GSX_ERR_INVALID_ARGUMENT, "rows = %d is not positive", im.rows);
    if (im.cols <= 0) return fail(GSX_ERR_INVALID_ARGUMENT, "cols = %d is not positive", im.cols);
    const int64_t need = 3 * (int64_t)im.cols;
    if (im.image_stride < need)
        return fail(GSX_ERR_INVALID_ARGUMENT, "image_row_stride %lld is below 3 cols = %lld", (long long)im.image_stride, (long long)need);
    if (im.target_stride < need)
        return fail(GSX_ERR_INVALID_ARGUMENT, "target_row_stride %lld is below 3 cols = %lld", (long long)im.target_stride, (long long)need);
    if (im.grad && im.grad_stride < need)
        return fail(GSX_ERR_INVALID_ARGUMENT, "grad_row_stride %lld is below 3 cols = %lld", (long long)im.grad_stride, (long long)need);
    return GSX_OK;
}
static int check_lambda_dssim(float lambda_dssim) {
    if (!(lambda_dssim >= 0.0f && lambda_dssim <= 1.0f))      // (a NaN fails both comparisons)
        return fail(GSX_ERR_INVALID_ARGUMENT, "lambda_dssim %g is outside [0, 1]", (double)lambda_dssim);
    return GSX_OK;
}

int gsx_photometric_loss(const float *image, int64_t image_row_stride, const float *target, int64_t target_row_stride,
                         int32_t rows, int32_t cols, float lambda_dssim, float *loss_out, float *grad_image,
                         int64_t grad_row_stride, void *workspace, size_t workspace_bytes, void *stream) {
    const gsx::LossImages im{image, target, grad_image, image_row_stride, target_row_stride, grad_row_stride, rows, cols};
    int rc = check_loss_images(im, loss_out);
    if (rc == GSX_OK) rc = check_lambda_dssim(lambda_dssim);
    if (rc != GSX_OK) return rc;
    LossCarve c;
    if (!loss_carve(rows, cols, grad_image != nullptr, c))
        return fail(GSX_ERR_INVALID_ARGUMENT, "rows x cols = %d x %d is more than 2^31 - 1 tiles of %d x %d", rows, cols, kLossTile, kLossTile);
    rc = check_sized_workspace(workspace, workspace_bytes, c.total, "gsx_photometric_loss_workspace_bytes(%d, %d, %d)", rows, cols,
                               grad_image ? 1 : 0);
    if (rc != GSX_OK) return rc;
    GSX_HIP(gsx::launch_photometric_loss(im, lambda_dssim, loss_out, (char *)workspace, c, (hipStream_t)stream));
    return GSX_OK;
}

size_t gsx_photometric_loss_weighted_workspace_bytes(int32_t rows, int32_t cols, int32_t with_grad) {
    LossWeightedCarve c;
    return loss_weighted_carve(rows, cols, with_grad != 0, c) ? c.total : 0;
}

int gsx_photometric_loss_weighted(const float *image, int64_t image_row_stride, const float *target, int64_t target_row_stride,
                                  const float *weight, int64_t weight_row_stride, const float *exposure, int32_t rows,
                                  int32_t cols, float lambda_dssim, float *loss_out, float *grad_image, int64_t grad_row_stride,
                                  float *grad_exposure, void *workspace, size_t workspace_bytes, void *stream) {
    const gsx::LossImages im{image, target, grad_image, image_row_stride, target_row_stride, grad_row_stride, rows, cols};
    int rc = check_loss_images(im, loss_out);
    if (rc != GSX_OK) return rc;
    if (weight && weight_row_stride < (int64_t)cols)
        return fail(GSX_ERR_INVALID_ARGUMENT, "weight_row_stride %lld is below cols = %d", (long long)weight_row_stride, cols);
    if (grad_exposure && !exposure) return fail(GSX_ERR_INVALID_ARGUMENT, "grad_exposure without exposure");
    if (grad_exposure && !grad_image) return fail(GSX_ERR_INVALID_ARGUMENT, "grad_exposure without grad_image");
    rc = check_lambda_dssim(lambda_dssim);
    if (rc != GSX_OK) return rc;
    LossWeightedCarve c;
    if (!loss_weighted_carve(rows, cols, grad_image != nullptr, c))
        return fail(GSX_ERR_INVALID_ARGUMENT, "rows x cols = %d x %d is more than 2^31 - 1 tiles of %d x %d", rows, cols, kLossTile, kLossTile);
    rc = check_sized_workspace(workspace, workspace_bytes, c.total, "gsx_photometric_loss_weighted_workspace_bytes(%d, %d, %d)", rows,
                               cols, grad_image ? 1 : 0);
    if (rc != GSX_OK) return rc;
    if (!weight && !exposure) {     // the kernels and the bits of gsx_photometric_loss; the carve starts with its carve
        GSX_HIP(gsx::launch_photometric_loss(im, lambda_dssim, loss_out, (char *)workspace, c.base, (hipStream_t)stream));
        GSX_HIP(gsx::launch_loss_weight_sum(rows, cols, loss_out, (hipStream_t)stream));
        return GSX_OK;
    }
    const gsx::LossWeights wt{weight, weight_row_stride, exposure, grad_exposure};
    GSX_HIP(gsx::launch_photometric_loss_weighted(im, wt, lambda_dssim, loss_out, (char *)workspace, c, (hipStream_t)stream));
    return GSX_OK;
}

int gsx_adam_step(const GsxAdamGroup *groups, int32_t n_groups, int64_t n, int64_t step, float beta1, float beta2, float eps,
                  uint32_t flags, void *stream) {
    if (!groups) return fail(GSX_ERR_INVALID_ARGUMENT, "groups is NULL");
    if (n_groups < 1 || n_groups > GSX_ADAM_MAX_GROUPS)
        return fail(GSX_ERR_INVALID_ARGUMENT, "n_groups = %d is outside 1 .. %d", n_groups, GSX_ADAM_MAX_GROUPS);
    if (n < 0) return fail(GSX_ERR_INVALID_ARGUMENT, "n = %lld is negative", (long long)n);
    if (n > (int64_t)0x7fffffff * kAdamRows) return fail(GSX_ERR_INVALID_ARGUMENT, "n = %lld is more than 2^31 - 1 blocks of %d rows", (long long)n, kAdamRows);
    if (step < 1) return fail(GSX_ERR_INVALID_ARGUMENT, "step = %lld is below 1", (long long)step);
    if (!(beta1 >= 0.0f && beta1 < 1.0f)) return fail(GSX_ERR_INVALID_ARGUMENT, "beta1 %g is outside [0, 1)", (double)beta1);   // (a NaN fails both)
    if (!(beta2 >= 0.0f && beta2 < 1.0f)) return fail(GSX_ERR_INVALID_ARGUMENT, "beta2 %g is outside [0, 1)", (double)beta2);
    if (!(eps >= 0.0f && eps <= FLT_MAX)) return fail(GSX_ERR_INVALID_ARGUMENT, "eps %g is negative or not finite", (double)eps);
    if (flags & ~GSX_ADAM_SKIP_ZERO_ROWS) return fail(GSX_ERR_INVALID_ARGUMENT, "flags 0x%x has unknown bits", flags);
    AdamArgs a;
    memset(&a, 0, sizeof a);
    for (int i = 0; i < n_groups; ++i) {
        const GsxAdamGroup &g = groups[i];
        if (g.width <= 0 || g.width > kAdamMaxWidth)
            return fail(GSX_ERR_INVALID_ARGUMENT, "groups[%d].width = %d is outside 1 .. %d", i, g.width, kAdamMaxWidth);
        if (g.transform != GSX_ADAM_LINEAR && g.transform != GSX_ADAM_LOG)
            return fail(GSX_ERR_INVALID_ARGUMENT, "groups[%d].transform = %d is unknown", i, g.transform);
        if (g.reserved != 0.0f) return fail(GSX_ERR_INVALID_ARGUMENT, "groups[%d].reserved is not 0", i);
        if (!(g.lr >= 0.0f && g.lr <= FLT_MAX)) return fail(GSX_ERR_INVALID_ARGUMENT, "groups[%d].lr %g is negative or not finite", i, (double)g.lr);
        if (n > 0) {
            if (!g.param) return fail(GSX_ERR_INVALID_ARGUMENT, "groups[%d].param is NULL", i);
            if (!g.grad) return fail(GSX_ERR_INVALID_ARGUMENT, "groups[%d].grad is NULL", i);
            if (!g.exp_avg) return fail(GSX_ERR_INVALID_ARGUMENT, "groups[%d].exp_avg is NULL", i);
            if (!g.exp_avg_sq) return fail(GSX_ERR_INVALID_ARGUMENT, "groups[%d].exp_avg_sq is NULL", i);
        }
        const uintptr_t bits = reinterpret_cast<uintptr_t>(g.param) | reinterpret_cast<uintptr_t>(g.grad) |
                               reinterpret_cast<uintptr_t>(g.exp_avg) | reinterpret_cast<uintptr_t>(g.exp_avg_sq);
        // the host scalars: once per call, in double, rounded to float (include/gsx.h)
        a.group[i] = AdamGroupArgs{g.param, g.grad, g.exp_avg, g.exp_avg_sq, g.width, g.transform == GSX_ADAM_LOG,
                                   (float)((double)g.lr / (1.0 - pow((double)beta1, (double)step))), (bits & 15u) == 0};
    }
    if (n == 0) return GSX_OK;
    a.n = n;
    a.n_groups = n_groups;
    a.beta1 = beta1;
    a.beta2 = beta2;
    a.c1 = (float)(1.0 - (double)beta1);
    a.c2 = (float)(1.0 - (double)beta2);
    a.s2 = (float)sqrt(1.0 - pow((double)beta2, (double)step));
    a.eps = eps;
    GSX_HIP(gsx::launch_adam(a, (flags & GSX_ADAM_SKIP_ZERO_ROWS) != 0, (hipStream_t)stream));
    return GSX_OK;
}

int gsx_transform_gaussians(float *points, float *scales, float *quaternions, float *sh, int32_t sh_degree, int64_t n,
                            const GsxTransform *transform, void *stream) {
    if (n < 0) return fail(GSX_ERR_INVALID_ARGUMENT, "n = %lld is negative", (long long)n);
    if (n > (int64_t)0x7fffffff * kTransformRows)
        return fail(GSX_ERR_INVALID_ARGUMENT, "n = %lld is more than 2^31 - 1 blocks of %d rows", (long long)n, kTransformRows);
    if (sh_degree < 0 || sh_degree > 3) return fail(GSX_ERR_INVALID_ARGUMENT, "sh_degree = %d is outside 0..3", sh_degree);
    if (!transform) return fail(GSX_ERR_INVALID_ARGUMENT, "transform is NULL");
    static_assert(sizeof(GsxTransform) == 100 * sizeof(float), "GsxTransform is 100 floats without padding");
    const struct { const char *name; const float *v; int count; } fields[] = {
        {"R", transform->R, 9},   {"s", &transform->s, 1},   {"t", transform->t, 3},   {"q_R", transform->q_R, 4},
        {"M1", transform->M1, 9}, {"M2", transform->M2, 25}, {"M3", transform->M3, 49}};
    for (const auto &f : fields)
        for (int i = 0; i < f.count; ++i)
            if (!(f.v[i] >= -FLT_MAX && f.v[i] <= FLT_MAX))         // (a NaN fails both)
                return fail(GSX_ERR_INVALID_ARGUMENT, "transform->%s[%d] = %g is not finite", f.name, i, (double)f.v[i]);
    if (!(transform->s > 0.0f)) return fail(GSX_ERR_INVALID_ARGUMENT, "transform->s = %g is not positive", (double)transform->s);
    if (n == 0) return GSX_OK;
    if (!points) return fail(GSX_ERR_INVALID_ARGUMENT, "points is NULL");
    if (!scales) return fail(GSX_ERR_INVALID_ARGUMENT, "scales is NULL");
    if (!quaternions) return fail(GSX_ERR_INVALID_ARGUMENT, "quaternions is NULL");
    if (sh_degree > 0 && !sh) return fail(GSX_ERR_INVALID_ARGUMENT, "sh is NULL with sh_degree = %d", sh_degree);
    TransformArgs a;
    memset(&a, 0, sizeof a);
    a.points = points;
    a.scales = scales;
    a.quats = quaternions;
    a.sh = sh_degree > 0 ? sh : nullptr;
    a.n = n;
    a.vec = (reinterpret_cast<uintptr_t>(sh) & 15u) == 0;
    a.T = *transform;
    GSX_HIP(gsx::launch_transform(a, sh_degree, (hipStream_t)stream));
    return GSX_OK;
}

int gsx_rectify_photo(const uint8_t *photo, int64_t photo_row_stride, const GsxLens *lens, const GsxPinhole *target,
                      int32_t samples, float *image_out, float *weight_out, void *stream) {
    if (!photo) return fail(GSX_ERR_INVALID_ARGUMENT, "photo is NULL");
    if (!lens) return fail(GSX_ERR_INVALID_ARGUMENT, "lens is NULL");
    if (!target) return fail(GSX_ERR_INVALID_ARGUMENT, "target is NULL");
    if (!image_out) return fail(GSX_ERR_INVALID_ARGUMENT, "image_out is NULL");
    if (samples < 1 || samples > 8) return fail(GSX_ERR_INVALID_ARGUMENT, "samples = %d is outside 1..8", samples);
    if (lens->width < 1 || lens->height < 1 || lens->width > kRectifyMaxSize || lens->height > kRectifyMaxSize)
        return fail(GSX_ERR_INVALID_ARGUMENT, "lens size %d x %d is outside 1..%d", lens->width, lens->height, kRectifyMaxSize);
    if (target->width < 1 || target->height < 1 || target->width > kRectifyMaxSize || target->height > kRectifyMaxSize)
        return fail(GSX_ERR_INVALID_ARGUMENT, "target size %d x %d is outside 1..%d", target->width, target->height, kRectifyMaxSize);
    if (photo_row_stride < (int64_t)3 * lens->width)
        return fail(GSX_ERR_INVALID_ARGUMENT, "photo_row_stride = %lld is below 3 * width = %lld", (long long)photo_row_stride,
                    (long long)3 * lens->width);
    static const char *const refused[] = {"OPENCV_FISHEYE", "FULL_OPENCV", "FOV", "SIMPLE_RADIAL_FISHEYE", "RADIAL_FISHEYE",
                                          "THIN_PRISM_FISHEYE"};
    if (lens->model > GSX_LENS_OPENCV && lens->model <= GSX_LENS_OPENCV + 6)
        return fail(GSX_ERR_UNSUPPORTED, "lens model %d (%s) is not supported: SIMPLE_PINHOLE, PINHOLE, SIMPLE_RADIAL, RADIAL, OPENCV",
                    lens->model, refused[lens->model - GSX_LENS_OPENCV - 1]);
    if (lens->model < GSX_LENS_SIMPLE_PINHOLE || lens->model > GSX_LENS_OPENCV)
        return fail(GSX_ERR_INVALID_ARGUMENT, "lens model %d is unknown", lens->model);
    RectifyArgs a;
    memset(&a, 0, sizeof a);
    const float *p = lens->params;
    int used = 0;       // params the model reads, COLMAP's order
    switch (lens->model) {
        case GSX_LENS_SIMPLE_PINHOLE: a.fxs = a.fys = p[0]; a.cxs = p[1]; a.cys = p[2]; used = 3; break;
        case GSX_LENS_PINHOLE: a.fxs = p[0]; a.fys = p[1]; a.cxs = p[2]; a.cys = p[3]; used = 4; break;
        case GSX_LENS_SIMPLE_RADIAL: a.fxs = a.fys = p[0]; a.cxs = p[1]; a.cys = p[2]; a.k1 = p[3]; used = 4; break;
        case GSX_LENS_RADIAL: a.fxs = a.fys = p[0]; a.cxs = p[1]; a.cys = p[2]; a.k1 = p[3]; a.k2 = p[4]; used = 5; break;
        default: a.fxs = p[0]; a.fys = p[1]; a.cxs = p[2]; a.cys = p[3]; a.k1 = p[4]; a.k2 = p[5]; a.p1 = p[6]; a.p2 = p[7]; used = 8; break;
    }
    const auto positive = [](float v) { return v > 0.0f && v <= FLT_MAX; };     // (a NaN fails both)
    if (!positive(a.fxs) || !positive(a.fys))
        return fail(GSX_ERR_INVALID_ARGUMENT, "lens focal length (%g, %g) is not positive and finite", (double)a.fxs, (double)a.fys);
    for (int i = 0; i < used; ++i)
        if (!(p[i] >= -FLT_MAX && p[i] <= FLT_MAX))
            return fail(GSX_ERR_INVALID_ARGUMENT, "lens->params[%d] = %g is not finite", i, (double)p[i]);
    if (!positive(target->fx) || !positive(target->fy))
        return fail(GSX_ERR_INVALID_ARGUMENT, "target focal length (%g, %g) is not positive and finite", (double)target->fx, (double)target->fy);
    if (!(target->cx >= -FLT_MAX && target->cx <= FLT_MAX && target->cy >= -FLT_MAX && target->cy <= FLT_MAX))
        return fail(GSX_ERR_INVALID_ARGUMENT, "target principal point (%g, %g) is not finite", (double)target->cx, (double)target->cy);
    a.photo = photo;
    a.row_stride = photo_row_stride;
    a.image = image_out;
    a.weight = weight_out;
    a.src_w = lens->width;
    a.src_h = lens->height;
    a.out_w = target->width;
    a.out_h = target->height;
    a.samples = samples;
    a.fx = target->fx;
    a.fy = target->fy;
    a.cx = target->cx;
    a.cy = target->cy;
    GSX_HIP(gsx::launch_rectify(a, (hipStream_t)stream));
    return GSX_OK;
}

int gsx_density_accumulate(const float *grad, int32_t width, int64_t n, float *grad_sum, uint32_t *seen, void *stream) {
    if (n < 0 || n > kDensityMaxRows) return fail(GSX_ERR_INVALID_ARGUMENT, "n = %lld is outside 0 .. 2^30", (long long)n);
    if (width < 1 || width > kDensityMaxWidth)
        return fail(GSX_ERR_INVALID_ARGUMENT, "width = %d is outside 1 .. %d", width, kDensityMaxWidth);
    if (n > 0) {
        if (!grad) return fail(GSX_ERR_INVALID_ARGUMENT, "grad is NULL");
        if (!grad_sum) return fail(GSX_ERR_INVALID_ARGUMENT, "grad_sum is NULL");
        if (!seen) return fail(GSX_ERR_INVALID_ARGUMENT, "seen is NULL");
    }
    GSX_HIP(gsx::launch_density_accumulate(grad, width, n, grad_sum, seen, (hipStream_t)stream));
    return GSX_OK;
}

int gsx_density_accumulate_screen(const float *grad_means2d, const float *screen_radius, int64_t n, float *grad_sum,
                                  uint32_t *seen, float *radius_max, void *stream) {
    if (n < 0 || n > kDensityMaxRows) return fail(GSX_ERR_INVALID_ARGUMENT, "n = %lld is outside 0 .. 2^30", (long long)n);
    if (n > 0) {
        if (!grad_means2d) return fail(GSX_ERR_INVALID_ARGUMENT, "grad_means2d is NULL");
        if (!screen_radius) return fail(GSX_ERR_INVALID_ARGUMENT, "screen_radius is NULL");
        if (!grad_sum) return fail(GSX_ERR_INVALID_ARGUMENT, "grad_sum is NULL");
        if (!seen) return fail(GSX_ERR_INVALID_ARGUMENT, "seen is NULL");
        if (!radius_max) return fail(GSX_ERR_INVALID_ARGUMENT, "radius_max is NULL");
    }
    GSX_HIP(gsx::launch_density_accumulate_screen(grad_means2d, screen_radius, n, grad_sum, seen, radius_max, (hipStream_t)stream));
    return GSX_OK;
}

size_t gsx_density_workspace_bytes(int64_t n) {
    DensityCarve c;
    return density_carve(n, c) ? c.total : 0;
}

namespace {
// n and the workspace of gsx_density_plan / gsx_density_apply
int check_density_workspace(int64_t n, const void *workspace, size_t workspace_bytes, DensityCarve &c) {
    if (!density_carve(n, c)) return fail(GSX_ERR_INVALID_ARGUMENT, "n = %lld is outside 0 .. 2^30", (long long)n);
    return check_sized_workspace(workspace, workspace_bytes, c.total, "gsx_density_workspace_bytes(%lld)", (long long)n);
}

// gsx_density_plan (radius_max == nullptr, prune_radius = +inf) and gsx_density_plan_screen: one body
int density_plan(const float *grad_sum, const uint32_t *seen, const float *scales, const float *opacity_logit,
                 const float *radius_max, float prune_radius, bool screen, int64_t n, const GsxDensityRules *rules, void *workspace,
                 size_t workspace_bytes, int64_t *counts_host, void *stream) {
    if (!rules) return fail(GSX_ERR_INVALID_ARGUMENT, "rules is NULL");
    if (!counts_host) return fail(GSX_ERR_INVALID_ARGUMENT, "counts_host is NULL");
    if (rules->flags != 0u) return fail(GSX_ERR_INVALID_ARGUMENT, "rules->flags 0x%x has unknown bits", rules->flags);
    if (!(rules->split_shrink > 0.0f && rules->split_shrink <= FLT_MAX))
        return fail(GSX_ERR_INVALID_ARGUMENT, "rules->split_shrink %g is not a positive finite number", (double)rules->split_shrink);
    if (prune_radius != prune_radius) return fail(GSX_ERR_INVALID_ARGUMENT, "prune_radius is NaN");
    DensityCarve c;
    const int rc = check_density_workspace(n, workspace, workspace_bytes, c);
    if (rc != GSX_OK) return rc;
    if (n > 0) {
        if (!grad_sum) return fail(GSX_ERR_INVALID_ARGUMENT, "grad_sum is NULL");
        if (!seen) return fail(GSX_ERR_INVALID_ARGUMENT, "seen is NULL");
        if (!scales) return fail(GSX_ERR_INVALID_ARGUMENT, "scales is NULL");
        if (!opacity_logit) return fail(GSX_ERR_INVALID_ARGUMENT, "opacity_logit is NULL");
    }
    for (int i = 0; i < 4; ++i) counts_host[i] = 0;
    if (n == 0) return GSX_OK;
    hipStream_t s = (hipStream_t)stream;
    if (screen)
        GSX_HIP(gsx::launch_density_plan_screen(grad_sum, seen, scales, opacity_logit, radius_max, prune_radius, n, *rules,
                                                (char *)workspace, c, s));
    else
        GSX_HIP(gsx::launch_density_plan(grad_sum, seen, scales, opacity_logit, n, *rules, (char *)workspace, c, s));
    GSX_HIP(hipMemcpyAsync(counts_host, (const char *)workspace + 8, 4 * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    GSX_HIP(hipStreamSynchronize(s));
    return GSX_OK;
}
}  // namespace

int gsx_density_plan(const float *grad_sum, const uint32_t *seen, const float *scales, const float *opacity_logit, int64_t n,
                     const GsxDensityRules *rules, void *workspace, size_t workspace_bytes, int64_t *counts_host, void *stream) {
    return density_plan(grad_sum, seen, scales, opacity_logit, nullptr, INFINITY, false, n, rules, workspace, workspace_bytes,
                        counts_host, stream);
}

int gsx_density_plan_screen(const float *grad_sum, const uint32_t *seen, const float *scales, const float *opacity_logit,
                            const float *radius_max, float prune_radius, int64_t n, const GsxDensityRules *rules, void *workspace,
                            size_t workspace_bytes, int64_t *counts_host, void *stream) {
    return density_plan(grad_sum, seen, scales, opacity_logit, radius_max, prune_radius, true, n, rules, workspace,
                        workspace_bytes, counts_host, stream);
}

int gsx_density_plan_contribution(const float *weight_max, const uint32_t *views, float threshold, int64_t n, void *workspace,
                                  size_t workspace_bytes, int64_t *counts_host, void *stream) {
    if (!counts_host) return fail(GSX_ERR_INVALID_ARGUMENT, "counts_host is NULL");
    if (!(threshold >= 0.0f)) return fail(GSX_ERR_INVALID_ARGUMENT, "threshold %g is NaN or negative", (double)threshold);
    DensityCarve c;
    const int rc = check_density_workspace(n, workspace, workspace_bytes, c);
    if (rc != GSX_OK) return rc;
    if (n > 0 && !weight_max) return fail(GSX_ERR_INVALID_ARGUMENT, "weight_max is NULL");
    for (int i = 0; i < 4; ++i) counts_host[i] = 0;
    if (n == 0) return GSX_OK;
    hipStream_t s = (hipStream_t)stream;
    GSX_HIP(gsx::launch_density_plan_contribution(weight_max, views, threshold, n, (char *)workspace, c, s));
    GSX_HIP(hipMemcpyAsync(counts_host, (const char *)workspace + 8, 4 * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    GSX_HIP(hipStreamSynchronize(s));
    return GSX_OK;
}

int gsx_density_apply(const GsxDensityGroup *groups, int32_t n_groups, int64_t n, int64_t n_out, const float *noise,
                      int32_t *source_row, void *workspace, size_t workspace_bytes, void *stream) {
    if (!groups) return fail(GSX_ERR_INVALID_ARGUMENT, "groups is NULL");
    if (n_groups < 1 || n_groups > GSX_DENSITY_MAX_GROUPS)
        return fail(GSX_ERR_INVALID_ARGUMENT, "n_groups = %d is outside 1 .. %d", n_groups, GSX_DENSITY_MAX_GROUPS);
    DensityCarve c;
    const int rc = check_density_workspace(n, workspace, workspace_bytes, c);
    if (rc != GSX_OK) return rc;
    if (n_out < 0 || n_out > 2 * n) return fail(GSX_ERR_INVALID_ARGUMENT, "n_out = %lld is outside 0 .. 2 n = %lld", (long long)n_out, (long long)(2 * n));
    DensityArgs a;
    memset(&a, 0, sizeof a);
    int at[5] = {-1, -1, -1, -1, -1};       // by role: the group that has it
    for (int i = 0; i < n_groups; ++i) {
        const GsxDensityGroup &g = groups[i];
        if (g.width < 1 || g.width > kDensityMaxWidth)
            return fail(GSX_ERR_INVALID_ARGUMENT, "groups[%d].width = %d is outside 1 .. %d", i, g.width, kDensityMaxWidth);
        if (g.role < GSX_DENSITY_COPY || g.role > GSX_DENSITY_QUATS)
            return fail(GSX_ERR_INVALID_ARGUMENT, "groups[%d].role = %d is unknown", i, g.role);
        if (g.role >= GSX_DENSITY_POINTS) {
            static const char *const names[] = {"", "", "POINTS", "SCALES", "QUATS"};
            if (at[g.role] >= 0)
                return fail(GSX_ERR_INVALID_ARGUMENT, "groups[%d].role: a second %s group (groups[%d] is one)", i, names[g.role], at[g.role]);
            const int want = g.role == GSX_DENSITY_QUATS ? 4 : 3;
            if (g.width != want)
                return fail(GSX_ERR_INVALID_ARGUMENT, "groups[%d].width = %d: a %s group has width %d", i, g.width, names[g.role], want);
            at[g.role] = i;
        }
        if (n > 0 && !g.src) return fail(GSX_ERR_INVALID_ARGUMENT, "groups[%d].src is NULL", i);
        if (n_out > 0 && !g.dst) return fail(GSX_ERR_INVALID_ARGUMENT, "groups[%d].dst is NULL", i);
        if (g.dst && g.dst == g.src) return fail(GSX_ERR_INVALID_ARGUMENT, "groups[%d].dst equals src: the rewrite is out of place", i);
        a.group[i] = DensityGroupArgs{g.src, g.dst, g.width, g.role};
    }
    if (at[GSX_DENSITY_POINTS] >= 0) {
        if (at[GSX_DENSITY_SCALES] < 0 || at[GSX_DENSITY_QUATS] < 0)
            return fail(GSX_ERR_INVALID_ARGUMENT, "groups[%d].role: a POINTS group needs a SCALES and a QUATS group in the same call",
                        at[GSX_DENSITY_POINTS]);
        if (!noise) return fail(GSX_ERR_INVALID_ARGUMENT, "noise is NULL with a POINTS group");
        a.scales = groups[at[GSX_DENSITY_SCALES]].src;
        a.quats = groups[at[GSX_DENSITY_QUATS]].src;
        a.noise = noise;
    }
    if (n == 0 || n_out == 0) return GSX_OK;
    hipStream_t s = (hipStream_t)stream;
    int64_t planned[2] = {-1, -1};          // the header's n and n_out
    GSX_HIP(hipMemcpyAsync(planned, workspace, sizeof planned, hipMemcpyDeviceToHost, s));
    GSX_HIP(hipStreamSynchronize(s));
    if (planned[0] != n) return fail(GSX_ERR_INVALID_ARGUMENT, "n = %lld, the plan in workspace is of %lld rows", (long long)n, (long long)planned[0]);
    if (planned[1] != n_out)
        return fail(GSX_ERR_INVALID_ARGUMENT, "n_out = %lld, the plan in workspace gives %lld rows", (long long)n_out, (long long)planned[1]);
    a.action = reinterpret_cast<const uint8_t *>((const char *)workspace + c.action);
    a.prefix = reinterpret_cast<const uint32_t *>((const char *)workspace + c.prefix);
    a.shrink = reinterpret_cast<const float *>((const char *)workspace + kDensityShrinkAt);
    a.source_row = source_row;
    a.n = n;
    a.n_groups = n_groups;
    GSX_HIP(gsx::launch_density_apply(a, n_out, s));
    return GSX_OK;
}

int gsx_mcmc_regularize(const float *opacity, const float *scales, int64_t n, float lambda_opacity, float lambda_scale,
                        float *grad_opacity, float *grad_scales, void *stream) {
    if (n < 0 || n > kMcmcMaxRows) return fail(GSX_ERR_INVALID_ARGUMENT, "n = %lld is outside 0 .. 2^30", (long long)n);
    if (!(lambda_opacity >= 0.0f && lambda_opacity <= FLT_MAX))     // (a NaN fails both comparisons)
        return fail(GSX_ERR_INVALID_ARGUMENT, "lambda_opacity %g is negative or not finite", (double)lambda_opacity);
    if (!(lambda_scale >= 0.0f && lambda_scale <= FLT_MAX))
        return fail(GSX_ERR_INVALID_ARGUMENT, "lambda_scale %g is negative or not finite", (double)lambda_scale);
    if (n > 0 && lambda_opacity != 0.0f) {
        if (!opacity) return fail(GSX_ERR_INVALID_ARGUMENT, "opacity is NULL");
        if (!grad_opacity) return fail(GSX_ERR_INVALID_ARGUMENT, "grad_opacity is NULL");
    }
    if (n > 0 && lambda_scale != 0.0f) {
        if (!scales) return fail(GSX_ERR_INVALID_ARGUMENT, "scales is NULL");
        if (!grad_scales) return fail(GSX_ERR_INVALID_ARGUMENT, "grad_scales is NULL");
    }
    if (n == 0) return GSX_OK;
    gsx::McmcRegularizeArgs a;
    memset(&a, 0, sizeof a);
    uintptr_t bits = 0;
    if (lambda_opacity != 0.0f) {
        a.opacity = opacity;
        a.grad_opacity = grad_opacity;
        bits |= reinterpret_cast<uintptr_t>(opacity) | reinterpret_cast<uintptr_t>(grad_opacity);
    }
    if (lambda_scale != 0.0f) {
        a.scales = scales;
        a.grad_scales = grad_scales;
        bits |= reinterpret_cast<uintptr_t>(scales) | reinterpret_cast<uintptr_t>(grad_scales);
    }
    a.n = n;
    // the host scalars: once per call, in double, rounded to float (include/gsx.h)
    a.coef_opacity = (float)((double)lambda_opacity / (double)n);
    a.coef_scale = (float)((double)lambda_scale / (3.0 * (double)n));
    a.vec = (bits & 15u) == 0;
    GSX_HIP(gsx::launch_mcmc_regularize(a, (hipStream_t)stream));
    return GSX_OK;
}

int gsx_mcmc_perturb(float *points, const float *scales, const float *quaternions, const float *opacity, const float *noise,
                     int64_t n, float rate, float gate_k, float gate_x0, void *stream) {
    if (n < 0 || n > kMcmcMaxRows) return fail(GSX_ERR_INVALID_ARGUMENT, "n = %lld is outside 0 .. 2^30", (long long)n);
    if (!(rate >= 0.0f && rate <= FLT_MAX)) return fail(GSX_ERR_INVALID_ARGUMENT, "rate %g is negative or not finite", (double)rate);
    if (!(gate_k >= 0.0f && gate_k <= FLT_MAX)) return fail(GSX_ERR_INVALID_ARGUMENT, "gate_k %g is negative or not finite", (double)gate_k);
    if (!(gate_x0 >= -FLT_MAX && gate_x0 <= FLT_MAX)) return fail(GSX_ERR_INVALID_ARGUMENT, "gate_x0 %g is not finite", (double)gate_x0);
    if (n == 0) return GSX_OK;
    if (!points) return fail(GSX_ERR_INVALID_ARGUMENT, "points is NULL");
    if (!scales) return fail(GSX_ERR_INVALID_ARGUMENT, "scales is NULL");
    if (!quaternions) return fail(GSX_ERR_INVALID_ARGUMENT, "quaternions is NULL");
    if (!opacity) return fail(GSX_ERR_INVALID_ARGUMENT, "opacity is NULL");
    if (!noise) return fail(GSX_ERR_INVALID_ARGUMENT, "noise is NULL");
    const uintptr_t bits = reinterpret_cast<uintptr_t>(points) | reinterpret_cast<uintptr_t>(scales) |
                           reinterpret_cast<uintptr_t>(quaternions) | reinterpret_cast<uintptr_t>(opacity) |
                           reinterpret_cast<uintptr_t>(noise);
    const gsx::McmcPerturbArgs a{points, scales, quaternions, opacity, noise, n, rate, gate_k, gate_x0, (bits & 15u) == 0};
    GSX_HIP(gsx::launch_mcmc_perturb(a, (hipStream_t)stream));
    return GSX_OK;
}

size_t gsx_mcmc_workspace_bytes(int64_t n) {
    McmcCarve c;
    return mcmc_carve(n, c) ? c.total : 0;
}

int gsx_mcmc_plan(const float *opacity, int64_t n, float dead_logit, int64_t n_out, const double *uniforms, uint32_t *weights,
                  int32_t *source, uint32_t *count, void *workspace, size_t workspace_bytes, int64_t *counts_host, void *stream) {
    McmcCarve c;
    if (!mcmc_carve(n, c)) return fail(GSX_ERR_INVALID_ARGUMENT, "n = %lld is outside 0 .. 2^30", (long long)n);
    if (n_out < n || n_out > kMcmcMaxRows || (n == 0 && n_out != 0))
        return fail(GSX_ERR_INVALID_ARGUMENT, "n_out = %lld is outside n = %lld .. 2^30", (long long)n_out, (long long)n);
    if (dead_logit != dead_logit) return fail(GSX_ERR_INVALID_ARGUMENT, "dead_logit is NaN");
    if (!counts_host) return fail(GSX_ERR_INVALID_ARGUMENT, "counts_host is NULL");
    const int rc = check_sized_workspace(workspace, workspace_bytes, c.total, "gsx_mcmc_workspace_bytes(%lld)", (long long)n);
    if (rc != GSX_OK) return rc;
    if (n > 0) {
        if (!opacity) return fail(GSX_ERR_INVALID_ARGUMENT, "opacity is NULL");
        if (!uniforms) return fail(GSX_ERR_INVALID_ARGUMENT, "uniforms is NULL");
        if (!weights) return fail(GSX_ERR_INVALID_ARGUMENT, "weights is NULL");
        if (!source) return fail(GSX_ERR_INVALID_ARGUMENT, "source is NULL");
        if (!count) return fail(GSX_ERR_INVALID_ARGUMENT, "count is NULL");
    }
    for (int i = 0; i < 3; ++i) counts_host[i] = 0;
    if (n == 0) return GSX_OK;
    hipStream_t s = (hipStream_t)stream;
    const gsx::McmcPlanArgs a{opacity, uniforms, weights, count, source, n, n_out, dead_logit};
    GSX_HIP(gsx::launch_mcmc_plan(a, (char *)workspace, c, s));
    GSX_HIP(hipMemcpyAsync(counts_host, workspace, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    GSX_HIP(hipStreamSynchronize(s));
    counts_host[2] = n_out - n;
    return GSX_OK;
}

int gsx_mcmc_apply(const GsxDensityGroup *groups, int32_t n_groups, int64_t n, int64_t n_out, const int32_t *source,
                   const uint32_t *count, float min_opacity, void *stream) {
    if (!groups) return fail(GSX_ERR_INVALID_ARGUMENT, "groups is NULL");
    if (n_groups < 1 || n_groups > GSX_DENSITY_MAX_GROUPS)
        return fail(GSX_ERR_INVALID_ARGUMENT, "n_groups = %d is outside 1 .. %d", n_groups, GSX_DENSITY_MAX_GROUPS);
    if (n < 0 || n > kMcmcMaxRows) return fail(GSX_ERR_INVALID_ARGUMENT, "n = %lld is outside 0 .. 2^30", (long long)n);
    if (n_out < n || n_out > kMcmcMaxRows || (n == 0 && n_out != 0))
        return fail(GSX_ERR_INVALID_ARGUMENT, "n_out = %lld is outside n = %lld .. 2^30", (long long)n_out, (long long)n);
    if (!(min_opacity > 0.0f && min_opacity < 1.0f))        // (a NaN fails both comparisons)
        return fail(GSX_ERR_INVALID_ARGUMENT, "min_opacity %g is outside (0, 1)", (double)min_opacity);
    gsx::McmcApplyArgs a;
    memset(&a, 0, sizeof a);
    int at[4] = {-1, -1, -1, -1};           // by role: the group that has it
    for (int i = 0; i < n_groups; ++i) {
        const GsxDensityGroup &g = groups[i];
        if (g.width < 1 || g.width > gsx::kMcmcMaxWidth)
            return fail(GSX_ERR_INVALID_ARGUMENT, "groups[%d].width = %d is outside 1 .. %d", i, g.width, gsx::kMcmcMaxWidth);
        if (g.role < GSX_MCMC_COPY || g.role > GSX_MCMC_SCALES)
            return fail(GSX_ERR_INVALID_ARGUMENT, "groups[%d].role = %d is unknown", i, g.role);
        if (g.role >= GSX_MCMC_OPACITY) {
            static const char *const names[] = {"", "", "OPACITY", "SCALES"};
            if (at[g.role] >= 0)
                return fail(GSX_ERR_INVALID_ARGUMENT, "groups[%d].role: a second %s group (groups[%d] is one)", i, names[g.role], at[g.role]);
            const int want = g.role == GSX_MCMC_SCALES ? 3 : 1;
            if (g.width != want)
                return fail(GSX_ERR_INVALID_ARGUMENT, "groups[%d].width = %d: a %s group has width %d", i, g.width, names[g.role], want);
            at[g.role] = i;
        }
        if (n > 0 && !g.src) return fail(GSX_ERR_INVALID_ARGUMENT, "groups[%d].src is NULL", i);
        if (n_out > 0 && !g.dst) return fail(GSX_ERR_INVALID_ARGUMENT, "groups[%d].dst is NULL", i);
        if (g.dst && g.dst == g.src) return fail(GSX_ERR_INVALID_ARGUMENT, "groups[%d].dst equals src: the rewrite is out of place", i);
        a.group[i] = gsx::DensityGroupArgs{g.src, g.dst, g.width, g.role};
    }
    if (at[GSX_MCMC_SCALES] >= 0 && at[GSX_MCMC_OPACITY] < 0)
        return fail(GSX_ERR_INVALID_ARGUMENT, "groups[%d].role: a SCALES group needs an OPACITY group in the same call", at[GSX_MCMC_SCALES]);
    if (n == 0 || n_out == 0) return GSX_OK;
    if (!source) return fail(GSX_ERR_INVALID_ARGUMENT, "source is NULL");
    if (!count) return fail(GSX_ERR_INVALID_ARGUMENT, "count is NULL");
    a.source = source;
    a.count = count;
    a.opacity = at[GSX_MCMC_OPACITY] >= 0 ? groups[at[GSX_MCMC_OPACITY]].src : nullptr;
    a.n = n;
    a.n_out = n_out;
    a.n_groups = n_groups;
    a.min_opacity = min_opacity;
    GSX_HIP(gsx::launch_mcmc_apply(a, (hipStream_t)stream));
    return GSX_OK;
}

size_t gsx_knn3_workspace_bytes(int64_t n) {
    KnnCarve c;
    return knn_carve(n, c) ? c.total : 0;
}

int gsx_knn3(const float *points, int64_t n, const int32_t *order, int32_t rule, float *dist3, float *scale, int64_t *candidates,
             void *workspace, size_t workspace_bytes, void *stream) {
    KnnCarve c;
    if (!knn_carve(n, c)) return fail(GSX_ERR_INVALID_ARGUMENT, "n = %lld is outside 0 .. 2^30", (long long)n);
    if (rule != GSX_KNN_RULE_REFERENCE && rule != GSX_KNN_RULE_PUBLISHED)
        return fail(GSX_ERR_INVALID_ARGUMENT, "rule = %d is neither GSX_KNN_RULE_REFERENCE nor GSX_KNN_RULE_PUBLISHED", rule);
    if (!dist3 && !scale) return fail(GSX_ERR_INVALID_ARGUMENT, "dist3 and scale are both NULL");
    if (n == 0) {
        if (candidates) *candidates = 0;
        return GSX_OK;
    }
    if (!points) return fail(GSX_ERR_INVALID_ARGUMENT, "points is NULL");
    const int rc = check_sized_workspace(workspace, workspace_bytes, c.total, "gsx_knn3_workspace_bytes(%lld)", (long long)n);
    if (rc != GSX_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (candidates) GSX_HIP(hipMemsetAsync(workspace, 0, sizeof(uint64_t), s));
    GSX_HIP(gsx::launch_knn3(points, n, order, rule, dist3, scale, (char *)workspace, c, candidates != nullptr, s));
    if (candidates) {
        GSX_HIP(hipMemcpyAsync(candidates, workspace, sizeof(int64_t), hipMemcpyDeviceToHost, s));
        GSX_HIP(hipStreamSynchronize(s));
    }
    return GSX_OK;
}

int gsx_covariance_3d(const float *scales, const float *quats, int64_t n, float *covariance_out, void *stream) {
    if (n < 0) return fail(GSX_ERR_INVALID_ARGUMENT, "n is negative");
    if (n > 0 && (!scales || !quats || !covariance_out)) return fail(GSX_ERR_INVALID_ARGUMENT, "an array is NULL");
    GSX_HIP(gsx::launch_covariance3d(scales, quats, n, covariance_out, (hipStream_t)stream));
    return GSX_OK;
}

int gsx_covariance_2d(const GsxCamera *camera, const float *points, const float *covariance_3d, int64_t n,
                      float *covariance_2d_out, void *stream) {
    if (!camera) return fail(GSX_ERR_INVALID_ARGUMENT, "camera is NULL");
    if (n < 0) return fail(GSX_ERR_INVALID_ARGUMENT, "n is negative");
    if (n > 0 && (!points || !covariance_3d || !covariance_2d_out)) return fail(GSX_ERR_INVALID_ARGUMENT, "an array is NULL");
    GSX_HIP(gsx::launch_covariance2d(*camera, points, covariance_3d, n, covariance_2d_out, (hipStream_t)stream));
    return GSX_OK;
}

int gsx_project_points(const GsxCamera *camera, const float *means3d, int64_t n, float *points_out,
                       uint8_t *in_view_out, void *stream) {
    if (!camera) return fail(GSX_ERR_INVALID_ARGUMENT, "camera is NULL");
    if (n < 0) return fail(GSX_ERR_INVALID_ARGUMENT, "n is negative");
    if (n > 0 && (!means3d || !points_out || !in_view_out)) return fail(GSX_ERR_INVALID_ARGUMENT, "an array is NULL");
    GSX_HIP(gsx::launch_project_points(*camera, means3d, n, points_out, in_view_out, (hipStream_t)stream));
    return GSX_OK;
}

}  // extern "C"
