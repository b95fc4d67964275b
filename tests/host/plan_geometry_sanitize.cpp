// The third workspace mode of csrc/gsx_plan.h -- carve(.., kCarveGeometry), gsx_render_backward_geometry's -- under
// AddressSanitizer + UndefinedBehaviorSanitizer, with the invariants tests/host/plan_sanitize.cpp holds the other two
// modes to: regions disjoint, 256-byte aligned, inside [0, total) and large enough; the backward carve's regions at the
// backward carve's offsets (so the colour-only slots keep their layout) with the second slot array behind them; the
// bytes the workspace function asks for hold the pairs asked for, and the capacity derived from a buffer fits it.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include \
//       -I intro_to_gaussian_splatting_amd/csrc tests/host/plan_geometry_sanitize.cpp -o plan_geometry_sanitize
// (tests/test_geometry_backward_host.py does exactly this.)  Exit code 0 and "ok" = every invariant held.
#include <stdio.h>
#include <stdlib.h>

#include "gsx_plan.h"

using namespace gsx;
using namespace gsx::plan;

static long long g_checks = 0;
#define CHECK(cond)                                                                      \
    do {                                                                                 \
        ++g_checks;                                                                      \
        if (!(cond)) {                                                                   \
            fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond);    \
            exit(1);                                                                     \
        }                                                                                \
    } while (0)

static uint64_t rng_state = 0xD1B54A32D192ED03ull;
static uint64_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}
static int64_t rnd_in(int64_t lo, int64_t hi) { return lo + (int64_t)(rnd() % (uint64_t)(hi - lo + 1)); }

static void check_carve(int64_t n, int64_t cap, int64_t max_tiles) {
    const size_t temp = binning_temp_bytes(n, cap);
    const Carve c = carve(n, cap, max_tiles, temp, kCarveGeometry);
    const Carve b = carve(n, cap, max_tiles, temp, kCarveBackward);
    const size_t nn = (size_t)(n > 0 ? n : 1), cc = (size_t)(cap > 0 ? cap : 1), tt = (size_t)(max_tiles > 0 ? max_tiles : 1);
    struct R { size_t off, bytes; };
    const R regs[] = {{c.keys0, nn * 4}, {c.keys1, nn * 4}, {c.vals0, nn * 4}, {c.vals1, nn * 4},
                      {c.rec, nn * kRecordBytes}, {c.rect, nn * kTileRectBytes}, {c.rrect, nn * kTileRectBytes},
                      {c.bbox, nn * kBboxBytes}, {c.tkeys0, cc * 4}, {c.tkeys1, cc * 4}, {c.tvals0, cc * 4},
                      {c.tvals1, cc * 4}, {c.ranges, tt * kRangeBytes}, {c.longs, kMaxLongTiles * 4},
                      {c.counters, 64}, {c.temp, temp},
                      {c.raw, nn * kRecordBytes}, {c.rank_of, nn * 4}, {c.prefix, (nn + 1) * 4}, {c.bsum, (nn / 1024 + 2) * 4},
                      {c.slots, cc * 16}, {c.geo_slots, cc * kGeoSlotBytes}};
    size_t prev_end = 0;
    for (const R &r : regs) {
        CHECK(r.bytes > 0);
        CHECK(r.off % 256 == 0);
        CHECK(r.off >= prev_end);
        CHECK(r.off + r.bytes <= c.total);
        prev_end = r.off + r.bytes;
    }
    // the backward carve's regions where the backward carve has them: the colour-only slots keep their layout
    CHECK(c.keys0 == b.keys0 && c.rec == b.rec && c.rrect == b.rrect && c.tvals1 == b.tvals1 && c.ranges == b.ranges &&
          c.longs == b.longs && c.redo == b.redo && c.sched == b.sched && c.counters == b.counters && c.temp == b.temp &&
          c.raw == b.raw && c.rank_of == b.rank_of && c.prefix == b.prefix && c.bsum == b.bsum && c.slots == b.slots);
    CHECK(b.geo_slots == 0 && carve(n, cap, max_tiles, temp).geo_slots == 0);
    CHECK(c.geo_slots >= b.total && c.total >= b.total + cc * kGeoSlotBytes);
    CHECK(kGeoSlotBytes % 16 == 0);     // whole float4 stores
}

static void check_capacity(int64_t n, int64_t cap, int32_t w, int32_t h, int32_t tile) {
    const int64_t max_tiles = max_tiles_of(w, h, tile);
    const Carve want = carve(n, cap, max_tiles, binning_temp_bytes(n, cap), kCarveGeometry);
    const int64_t got = capacity_for(want.total, n, max_tiles, kCarveGeometry);
    CHECK(got >= cap);
    CHECK(got <= kMaxPairs);
    const Carve fit = carve(n, got, max_tiles, binning_temp_bytes(n, got), kCarveGeometry);
    CHECK(fit.total <= want.total);
    if (want.total > 4096) CHECK(capacity_for(want.total - 4096, n, max_tiles, kCarveGeometry) <= got);
    CHECK(capacity_for(0, n, max_tiles, kCarveGeometry) == -1);
    CHECK(cap == 0 || got == cap || carve(n, got + 1, max_tiles, binning_temp_bytes(n, got + 1), kCarveGeometry).total > want.total ||
          got == kMaxPairs);
    // a buffer sized for the colour-only backward holds fewer pairs in this mode, never more
    const Carve colour = carve(n, cap, max_tiles, binning_temp_bytes(n, cap), kCarveBackward);
    CHECK(capacity_for(colour.total, n, max_tiles, kCarveGeometry) <= capacity_for(colour.total, n, max_tiles, kCarveBackward));
    check_carve(n, got, max_tiles);
}

int main() {
    const int64_t ns[] = {0, 1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 100000, 1000000, 5000000, ((int64_t)1 << 31) - 1};
    const int64_t caps[] = {0, 1, 255, 256, 4096, 4097, 1000000, 30000000, ((int64_t)1 << 31) - 1};
    const int32_t tiles[] = {1, 2, 3, 8, 12, 16, 20, 32, 64};
    for (int64_t n : ns)
        for (int64_t cap : caps) {
            check_carve(n, cap, 1);
            check_carve(n, cap, max_tiles_of(1920, 1080, 16));
            check_carve(n, cap, max_tiles_of(3840, 2160, 16));
        }
    for (int64_t n : ns)
        for (int64_t cap : caps)
            for (int32_t tile : tiles) check_capacity(n, cap, 1920, 1080, tile);
    for (int i = 0; i < 2000; ++i) {
        const int64_t n = rnd_in(0, i % 7 == 0 ? ((int64_t)1 << 31) - 1 : 3000000);
        const int64_t cap = rnd_in(0, i % 5 == 0 ? ((int64_t)1 << 31) - 1 : 50000000);
        const int32_t w = (int32_t)rnd_in(1, 8192), h = (int32_t)rnd_in(1, 8192), tile = (int32_t)rnd_in(1, 64);
        check_capacity(n, cap, w, h, tile);
    }
    printf("ok: %lld checks\n", g_checks);
    return 0;
}
