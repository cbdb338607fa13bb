// The 2-(G)FSK modem's law (simplefe_amd/csrc/fsk_law.h) on the host, for a build with -fsanitize=address,undefined
// (tests/test_fsk_host.py builds and runs it).  A stand-alone program: it makes its own inputs from a fixed generator.  Every
// buffer is a heap block of exactly the size the contract names, so a store or a load one element outside is a report.
//   - fsk_cis: exactly (+-1, +-0) or (+-0, +-1) at the four quadrant phases; within 2 ulp(1) = 2.39e-7 of float64 cos / sin on
//     every 4099th phase and on the +-4096 neighbours of the eight multiples of 2^29; with the argument --all, on every one
//     of the 2^32 phases (run without the sanitizers: the figure in DESIGN.md 4.26 comes from there)
//   - the tile form of P[i] (the level sum of the symbols passed, from a count of set bits, plus the at most Q in flight)
//     against the defining sum over all k, for every sample of frames of several shapes
//   - the tree in its stride form against its statement, s[k] = s[2k] + s[2k+1] level by level on a padded copy
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../simplefe_amd/csrc/fsk_law.h"

using namespace sfe;

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_state >> 32);
}

#define CHECK(cond, ...)                       \
    do {                                       \
        if (!(cond)) {                         \
            printf("FAILED %s: ", #cond);      \
            printf(__VA_ARGS__);               \
            printf("\n");                      \
            return 1;                          \
        }                                      \
        checks++;                              \
    } while (0)

static long checks = 0;
static const double BAR = 2.0 * 1.1920928955078125e-7;

static double cis_err(uint32_t p)
{
    const FskC e = fsk_cis(p);
    const double a = 6.283185307179586476925 * (double)p / 4294967296.0;
    const double dc = fabs((double)e.r - cos(a)), ds = fabs((double)e.i - sin(a));
    return dc > ds ? dc : ds;
}

static int test_cis(bool all)
{
    static const float want[4][2] = {{1.0f, 0.0f}, {0.0f, 1.0f}, {-1.0f, 0.0f}, {0.0f, -1.0f}};
    for (uint32_t k = 0; k < 4; k++) {
        const FskC e = fsk_cis(k << 30);
        CHECK(fabsf(e.r) == fabsf(want[k][0]) && fabsf(e.i) == fabsf(want[k][1]), "quadrant %u: (%a, %a)", k, e.r, e.i);
        CHECK((want[k][0] == 0.0f || e.r == want[k][0]) && (want[k][1] == 0.0f || e.i == want[k][1]), "quadrant %u: signs", k);
    }
    double worst = 0.0;
    for (uint64_t p = 0; p < (1ull << 32); p += all ? 1 : 4099) {
        const double d = cis_err((uint32_t)p);
        if (d > worst) worst = d;
    }
    for (uint32_t m = 0; m < 8; m++)
        for (int d = -4096; d <= 4096; d++) {
            const double v = cis_err((m << 29) + (uint32_t)d);
            if (v > worst) worst = v;
        }
    CHECK(worst <= BAR, "worst |fsk_cis - float64| = %.4g above %.4g", worst, BAR);
    printf("fsk_cis: worst error %.4g of the bar %.4g on %s\n", worst, BAR, all ? "all 2^32 phases" : "every 4099th phase and the octant edges");
    return 0;
}

static int test_phase(int sps, int n_taps, int Lp, int n_bits)
{
    const int N = Lp + n_bits, Q = (n_taps + sps - 1) / sps, F = (N + Q - 1) * sps + 1;
    uint32_t *C = (uint32_t *)malloc(((size_t)n_taps + 1) * sizeof(uint32_t));
    uint8_t *pre = (uint8_t *)malloc(((size_t)Lp + 7) / 8), *row = (uint8_t *)malloc(((size_t)n_bits + 7) / 8);
    C[0] = 0;
    for (int j = 0; j < n_taps; j++) C[j + 1] = C[j] + (uint32_t)((int32_t)(rnd() >> 8) - (1 << 22));        // signed steps
    for (int j = 0; j < (Lp + 7) / 8; j++) pre[j] = (uint8_t)rnd();
    for (int j = 0; j < (n_bits + 7) / 8; j++) row[j] = (uint8_t)rnd();
    auto lev = [&](int k) { return 1 - 2 * (int)(k < Lp ? fsk_bit(pre, k) : fsk_bit(row, k - Lp)); };
    for (int i = 0; i < F; i++) {
        uint32_t def = 0;                                       // the defining sum over all k
        for (int k = 0; k < N; k++) {
            int t = i - k * sps;
            t = t < 0 ? 0 : (t > n_taps ? n_taps : t);
            def += lev(k) > 0 ? C[t] : 0u - C[t];
        }
        const int kp = fsk_passed(i, sps, n_taps, N);
        const int ones = fsk_ones(pre, kp < Lp ? kp : Lp) + fsk_ones(row, kp > Lp ? kp - Lp : 0);
        int flight = 0;
        const uint32_t tile = fsk_phase(i, sps, N, C[n_taps], kp - 2 * ones, kp, C, [&](int k) {
            flight++;
            return lev(k);
        });
        CHECK(tile == def, "sps %d n_taps %d Lp %d n_bits %d sample %d: %08x != %08x", sps, n_taps, Lp, n_bits, i, tile, def);
        CHECK(flight <= Q, "sample %d: %d symbols in flight, Q = %d", i, flight, Q);
        if (i == F - 1) CHECK(kp == N && flight == 0, "the last sample: every pulse has passed");
        if (i == 0) CHECK(def == 0, "P[0] = 0");
    }
    free(C);
    free(pre);
    free(row);
    return 0;
}

static int test_tree(int n)
{
    const int n2 = fsk_pow2(n);
    float *s = (float *)malloc((size_t)n2 * sizeof(float)), *w = (float *)malloc((size_t)n2 * sizeof(float));
    for (int k = 0; k < n2; k++) s[k] = w[k] = k < n ? (float)((double)rnd() / 4294967296.0 - 0.5) * (float)(1 + (rnd() & 1023)) : 0.0f;
    for (int len = n2; len > 1; len /= 2)                       // the statement
        for (int k = 0; k < len / 2; k++) w[k] = w[2 * k] + w[2 * k + 1];
    const float got = fsk_tree(s, n2);
    CHECK(memcmp(&got, &w[0], 4) == 0, "tree of %d: %a != %a", n, got, w[0]);
    free(s);
    free(w);
    return 0;
}

int main(int argc, char **argv)
{
    const bool all = argc > 1 && strcmp(argv[1], "--all") == 0;
    if (test_cis(all)) return 1;
    static const int shapes[][4] = {{4, 4, 8, 8}, {4, 12, 24, 64}, {8, 24, 24, 100}, {10, 40, 24, 257}, {64, 128, 16, 33},
                                    {2, 1, 2, 1}, {3, 7, 5, 19}, {5, 320, 9, 70}, {2, 128, 1024, 3}, {7, 3, 2, 40}};
    for (const auto &sh : shapes)
        if (test_phase(sh[0], sh[1], sh[2], sh[3])) return 1;
    static const int sizes[] = {1, 2, 3, 7, 8, 16, 24, 100, 1024};
    for (int n : sizes)
        if (test_tree(n)) return 1;
    CHECK(fsk_pow2(1) == 1 && fsk_pow2(24) == 32 && fsk_pow2(1024) == 1024 && fsk_pow2(1025) == 2048, "fsk_pow2");
    const FskFit f = fsk_fit(24, 3.0f, 2.0f, 0.5f, 4.0f);
    CHECK(f.dev == 1.5f && f.dc == (4.0f - 0.75f) / 24.0f && fsk_fit_ok(f.dev) && !fsk_fit_ok(0.0f) && !fsk_fit_ok(NAN) && !fsk_fit_ok(INFINITY), "the fit");
    printf("fsk law ok: %ld checks\n", checks);
    return 0;
}
