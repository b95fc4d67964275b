// The workspace arithmetic of gsx_mcmc_plan (intro_to_gaussian_splatting_amd/csrc/gsx_plan.h: mcmc_carve) under
// AddressSanitizer + UndefinedBehaviorSanitizer, swept over row counts up to the 2^30 limit.  No GPU, no HIP:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include \
//       -I intro_to_gaussian_splatting_amd/csrc tests/host/plan_mcmc_sanitize.cpp -o plan_mcmc_sanitize \
//       && ./plan_mcmc_sanitize
// (tests/test_mcmc_host.py does exactly this.)  Exit code 0 and "ok" = every invariant held; the lines behind it are
// "n total" pairs the test compares with gsx_mcmc_workspace_bytes.
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

// Everything a carve promises, in 128-bit arithmetic so that the check itself cannot wrap.
static void check_carve(int64_t n) {
    typedef unsigned __int128 u128;
    McmcCarve c;
    const bool ok = mcmc_carve(n, c);
    CHECK(ok == (n >= 0 && n <= kMcmcMaxRows));
    if (!ok) {
        CHECK(c.total == 0 && c.scan_blocks == 0);
        return;
    }
    const u128 nsb = ((u128)n + kMcmcScanRows - 1) / kMcmcScanRows;
    CHECK((u128)c.scan_blocks == nsb && nsb * kMcmcScanRows >= (u128)n && nsb <= ((u128)1 << 20));
    CHECK(c.prefix == kMcmcHeader && c.prefix >= 3 * sizeof(int64_t));      // the header holds n_dead, n_live, total
    CHECK(c.prefix % 256 == 0 && c.bsum % 256 == 0 && c.btally % 256 == 0 && c.total % 256 == 0);
    // every region holds what the kernels index in it, and ends before the next begins
    const u128 prefix_bytes = nsb * kMcmcScanRows * 4, bsum_bytes = (nsb + 1) * 8, tally_bytes = 2 * nsb * 4;
    CHECK((u128)c.bsum >= (u128)c.prefix + prefix_bytes && (u128)c.bsum < (u128)c.prefix + prefix_bytes + 256);
    CHECK((u128)c.btally >= (u128)c.bsum + bsum_bytes && (u128)c.btally < (u128)c.bsum + bsum_bytes + 256);
    CHECK((u128)c.total >= (u128)c.btally + tally_bytes && (u128)c.total < (u128)c.btally + tally_bytes + 256);
    CHECK((u128)c.total < ((u128)1 << 40));
    // the sums the kernels keep: a block's in-block prefix fits 32 bits, the total 2^52
    CHECK((u128)(kMcmcScanRows - 1) * ((u128)1 << 22) < ((u128)1 << 32));
    CHECK((u128)kMcmcMaxRows * ((u128)1 << 22) <= ((u128)1 << 52));
}

int main() {
    const int64_t edges[] = {INT64_MIN, -((int64_t)1 << 40), -1, 0, 1, 2, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049,
                             262143, 262144, 262145, 1000000, ((int64_t)1 << 30) - 1, (int64_t)1 << 30, ((int64_t)1 << 30) + 1,
                             (int64_t)1 << 31, (int64_t)1 << 40, INT64_MAX};
    for (int64_t n : edges) check_carve(n);
    for (int i = 0; i < 200000; ++i) {
        const int bits = (int)rnd_in(1, 31);
        check_carve(rnd_in(0, ((int64_t)1 << bits) - 1));
    }
    for (int i = 0; i < 20000; ++i) {       // both sides of every block boundary, and monotone
        const int64_t n = rnd_in(1, (1 << 20) - 1) * kMcmcScanRows;
        McmcCarve a, b, d;
        CHECK(mcmc_carve(n - 1, a) && mcmc_carve(n, b));
        CHECK(a.total == b.total && a.scan_blocks == b.scan_blocks);
        if (n < kMcmcMaxRows) {
            CHECK(mcmc_carve(n + 1, d));
            CHECK(d.total > b.total && d.scan_blocks == b.scan_blocks + 1);
        }
    }
    printf("ok: %lld checks\n", g_checks);
    const int64_t shown[] = {0, 1, 1024, 1025, 3000, 1000000, (int64_t)1 << 30};
    for (int64_t n : shown) {
        McmcCarve c;
        CHECK(mcmc_carve(n, c));
        printf("%lld %zu\n", (long long)n, c.total);
    }
    return 0;
}
