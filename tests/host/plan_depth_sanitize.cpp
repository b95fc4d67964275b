// The fifth workspace mode of csrc/gsx_plan.h -- carve(.., kCarveDepth), gsx_render_depth's and
// gsx_render_backward_depth's -- under AddressSanitizer + UndefinedBehaviorSanitizer, with the invariants
// tests/host/plan_camera_sanitize.cpp holds the fourth mode to: the geometry carve's regions at the geometry carve's
// offsets (so the slots keep their layout and the geometry workspace its size), no camera partials, the per-row depth
// array behind them, 256-byte aligned, inside [0, total) and large enough for one float per Gaussian; the capacity
// derived from a buffer fits it.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include \
//       -I intro_to_gaussian_splatting_amd/csrc tests/host/plan_depth_sanitize.cpp -o plan_depth_sanitize
// (tests/test_depth_host.py does exactly this.)  Exit code 0 and "ok" = every invariant held.
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

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}
static int64_t rnd_in(int64_t lo, int64_t hi) { return lo + (int64_t)(rnd() % (uint64_t)(hi - lo + 1)); }

static void check_carve(int64_t n, int64_t cap, int64_t max_tiles) {
    const size_t temp = binning_temp_bytes(n, cap);
    const Carve c = carve(n, cap, max_tiles, temp, kCarveDepth);
    const Carve g = carve(n, cap, max_tiles, temp, kCarveGeometry);
    const size_t cc = (size_t)(cap > 0 ? cap : 1), nn = (size_t)(n > 0 ? n : 1);
    // the geometry carve, byte for byte
    CHECK(c.keys0 == g.keys0 && c.rec == g.rec && c.rrect == g.rrect && c.tvals1 == g.tvals1 && c.ranges == g.ranges &&
          c.longs == g.longs && c.redo == g.redo && c.sched == g.sched && c.counters == g.counters && c.temp == g.temp &&
          c.raw == g.raw && c.rank_of == g.rank_of && c.prefix == g.prefix && c.bsum == g.bsum && c.slots == g.slots &&
          c.geo_slots == g.geo_slots);
    CHECK(c.cam_partials == 0);
    CHECK(g.zrow == 0 && carve(n, cap, max_tiles, temp, kCarveBackward).zrow == 0 && carve(n, cap, max_tiles, temp).zrow == 0 &&
          carve(n, cap, max_tiles, temp, kCarveCamera).zrow == 0);
    // the depths behind it: one float per Gaussian
    CHECK(c.zrow % 256 == 0);
    CHECK(c.zrow >= g.total && c.zrow >= c.geo_slots + cc * kGeoSlotBytes);
    CHECK(c.zrow + nn * sizeof(float) <= c.total);
    CHECK(c.total >= g.total + sizeof(float) && c.total - g.total <= nn * sizeof(float) + 255);
    // the second float4 of a pair's geometry slot holds (S5, Sz, 0, 0): the slot did not grow
    CHECK(kGeoSlotBytes == 32);
}

static void check_capacity(int64_t n, int64_t cap, int32_t w, int32_t h, int32_t tile) {
    const int64_t max_tiles = max_tiles_of(w, h, tile);
    const Carve want = carve(n, cap, max_tiles, binning_temp_bytes(n, cap), kCarveDepth);
    const int64_t got = capacity_for(want.total, n, max_tiles, kCarveDepth);
    CHECK(got >= cap);
    CHECK(got <= kMaxPairs);
    CHECK(carve(n, got, max_tiles, binning_temp_bytes(n, got), kCarveDepth).total <= want.total);
    CHECK(capacity_for(0, n, max_tiles, kCarveDepth) == -1);
    // a buffer sized for the geometry entry holds no more pairs in this mode
    const Carve geo = carve(n, cap, max_tiles, binning_temp_bytes(n, cap), kCarveGeometry);
    CHECK(capacity_for(geo.total, n, max_tiles, kCarveDepth) <= capacity_for(geo.total, n, max_tiles, kCarveGeometry));
    check_carve(n, got, max_tiles);
}

int main() {
    const int64_t ns[] = {0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 100000, 1000000, 5000000, ((int64_t)1 << 31) - 1};
    const int64_t caps[] = {0, 1, 255, 256, 4096, 4097, 1000000, 30000000, ((int64_t)1 << 31) - 1};
    const int32_t tiles[] = {1, 2, 3, 8, 12, 16, 20, 32, 64};
    for (int64_t n : ns)
        for (int64_t cap : caps) {
            check_carve(n, cap, 1);
            check_carve(n, cap, max_tiles_of(1920, 1080, 16));
        }
    for (int64_t n : ns)
        for (int64_t cap : caps)
            for (int32_t tile : tiles) check_capacity(n, cap, 1920, 1080, tile);
    for (int i = 0; i < 1000; ++i) {
        const int64_t n = rnd_in(0, i % 7 == 0 ? ((int64_t)1 << 31) - 1 : 3000000);
        const int64_t cap = rnd_in(0, i % 5 == 0 ? ((int64_t)1 << 31) - 1 : 50000000);
        const int32_t w = (int32_t)rnd_in(1, 8192), h = (int32_t)rnd_in(1, 8192), tile = (int32_t)rnd_in(1, 64);
        check_capacity(n, cap, w, h, tile);
    }
    printf("ok: %lld checks\n", g_checks);
    return 0;
}
