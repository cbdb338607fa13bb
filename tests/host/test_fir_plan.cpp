// test_fir_plan.cpp -- csrc/fir_plan.h alone, built by a plain host compiler under -fsanitize=address,undefined
// (tests/test_fir_plan_host.py).  The header is the only library file included -- it needs no HIP.
//   spectra     every table entry, read at the index the kernel reads it (thread t = k1 | k2 << 4, register k0, for bin
//               k2 + 16 k1 + 256 k0), against a direct long-double DFT of the zero-padded partition divided by 4096, real and
//               imaginary part each within 2^-23 of the largest |component| of that partition's spectrum: a float rounding
//               is at most 2^-24 relative and the double FFT's own error is nine orders below, so the bound is twice the
//               rounding.  EVERY one of the 4096 bins of every partition of every set is checked (no stride: the whole
//               program runs in under a second).  Each set has taps of its own, so a set that read another's row fails.
//   twiddles    tw1[k][t] = W_4096^(t k), tw1[k+3][t] = W_4096^(4 t k), tw2 likewise over 256, within one float rounding of
//               the long-double value; row 0 is zero.
//   planner     what tests/test_host_logic.py::test_fir_partition_plan asserts through the C ABI, directly; the history
//               length a handle carries; the tap counts one launch serves (the resampler builds general-rate tables there).
//   size class  at powers of two and their neighbours.
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "../../simplefe_amd/csrc/fir_plan.h"

using namespace sfe;

struct F2 {
    float x, y;
};

static int g_fails = 0, g_checks = 0;
static void expect_true(int line, bool ok)
{
    g_checks++;
    if (ok) return;
    g_fails++;
    if (g_fails < 40) printf("line %d: false\n", line);
}
#define TRUE(x) expect_true(__LINE__, (x))

static uint32_t g_seed = 12345;
static float rnd()          // in [-1, 1)
{
    g_seed = g_seed * 1664525u + 1013904223u;
    return (float)((int32_t)g_seed >> 8) / 8388608.0f;
}

static long double g_wr[4096], g_wi[4096];      // exp(-2 pi j q / 4096)

static double g_worst = 0.0;        // of all spectra, in units of 2^-24 of the partition's largest component
static void test_spectra(int n_taps, int cplx, int n_sets, int parts, int ovl)
{
    const int N = 4096, w = cplx ? 2 : 1;
    std::vector<float> taps((size_t)n_sets * n_taps * w);
    for (float &t : taps) t = rnd();
    const std::vector<F2> hs = fir_spectra<F2>(FirShape{n_taps, cplx, n_sets, parts, ovl}, taps.data());
    TRUE(hs.size() == (size_t)n_sets * parts * 4096);
    if (hs.size() != (size_t)n_sets * parts * 4096) return;
    std::vector<long double> re(N), im(N);
    for (int set = 0; set < n_sets; set++)
        for (int p = 0; p < parts; p++) {
            // the partition, zero-padded: taps [p ovl, (p + 1) ovl) of this set's row; a single partition holds them all
            const int first = parts == 1 ? 0 : p * ovl, count = parts == 1 ? n_taps : std::min(ovl, n_taps - first);
            TRUE(count >= 1 && count <= N);
            const float *row = taps.data() + (size_t)set * n_taps * w;
            long double big = 0.0L;
            for (int k = 0; k < N; k++) {
                long double sr = 0.0L, si = 0.0L;
                for (int n = 0; n < count; n++) {
                    const int q = (int)(((long long)n * k) & (N - 1));
                    const long double xr = row[(size_t)(first + n) * w], xi = cplx ? row[(size_t)(first + n) * w + 1] : 0.0L;
                    sr += xr * g_wr[q] - xi * g_wi[q];
                    si += xr * g_wi[q] + xi * g_wr[q];
                }
                re[k] = sr / N;
                im[k] = si / N;
                big = std::max(big, std::max(fabsl(re[k]), fabsl(im[k])));
            }
            const long double bound = ldexpl(big, -23);
            long double worst = 0.0L;
            for (int k0 = 0; k0 < 16; k0++)
                for (int k1 = 0; k1 < 16; k1++)
                    for (int k2 = 0; k2 < 16; k2++) {
                        const int t = k1 | (k2 << 4), bin = k2 + 16 * k1 + 256 * k0;
                        const F2 v = hs[(((size_t)set * parts + p) * 16 + k0) * 256 + t];
                        worst = std::max(worst, std::max(fabsl(v.x - re[bin]), fabsl(v.y - im[bin])));
                    }
            TRUE(big > 0.0L && worst <= bound);
            g_worst = std::max(g_worst, (double)(worst / ldexpl(big, -24)));
        }
}

static void test_twiddles()
{
    std::vector<F2> tw1(3, F2{9.0f, 9.0f}), tw2;
    fir_twiddles(tw1, tw2);
    TRUE(tw1.size() == 7 * 256 && tw2.size() == 7 * 16);
    if (tw1.size() != 7 * 256 || tw2.size() != 7 * 16) return;
    // one float rounding of the float64 value: 2^-24 relative; the float64 value itself lies within 2^-50 of the exact one
    // (the angle, up to 5 radians, is rounded to a double before the cosine), which counts only next to a zero crossing
    auto close = [](float got, long double want) { return fabsl(got - want) <= ldexpl(fabsl(want), -24) + ldexpl(1.0L, -50); };
    auto row = [&](const std::vector<F2> &tw, int len, int N) {
        const long double unit = -2.0L * acosl(-1.0L) / N;
        for (int t = 0; t < len; t++) {
            TRUE(tw[t].x == 0.0f && tw[t].y == 0.0f);           // row 0: not read, zero
            for (int k = 1; k < 4; k++) {
                const long double a = unit * (t * k);
                TRUE(close(tw[k * len + t].x, cosl(a)) && close(tw[k * len + t].y, sinl(a)));
                TRUE(close(tw[(k + 3) * len + t].x, cosl(4.0L * a)) && close(tw[(k + 3) * len + t].y, sinl(4.0L * a)));
            }
        }
    };
    row(tw1, 256, 4096);
    row(tw2, 16, 256);
}

struct Plan {
    int ovl, parts, adv;
    bool ok;
};
static Plan plan(int n)
{
    Plan p{0, 0, 0, false};
    p.ok = fir_choose_partition(n, &p.ovl, &p.parts);
    p.adv = 4096 - p.ovl;
    return p;
}
static bool is(const Plan &p, int ovl, int parts, int adv) { return p.ok && p.ovl == ovl && p.parts == parts && p.adv == adv; }

static void test_planner()
{
    TRUE(FIR_PLAN_N == 4096 && FIR_MAX_PARTS == 1024);
    TRUE(fir_single_overlap(1) == 256 && fir_single_overlap(2) == 256 && fir_single_overlap(257) == 256 && fir_single_overlap(258) == 512 &&
         fir_single_overlap(3841) == 3840 && fir_single_overlap(3842) == 4096);
    TRUE(is(plan(1), 256, 1, 3840) && is(plan(256), 256, 1, 3840) && is(plan(257), 256, 1, 3840));
    TRUE(is(plan(258), 512, 1, 3584) && plan(551).parts == 1 && is(plan(2001), 2048, 1, 2048));
    std::vector<int> grid;
    for (int n = 1; n < 9000; n += 37) grid.push_back(n);
    for (int n : {3841, 3842, 4096, 8192, 65536, 245765, 1 << 20}) grid.push_back(n);
    std::sort(grid.begin(), grid.end());
    double prev = 0.0;
    for (int n : grid) {
        const Plan p = plan(n);
        TRUE(p.ok && p.ovl % 256 == 0 && 256 <= p.ovl && p.ovl < 4096);
        TRUE((p.parts == 1 && n <= p.ovl + 1) || (p.parts > 1 && (long long)p.parts * p.ovl >= n));
        TRUE(p.parts != 1 || p.ovl == fir_single_overlap(n));
        const double cost = (p.parts + 0.25 * (p.parts - 1)) / p.adv;
        const double single = n <= 3841 ? 1.0 / (4096 - 256 * ((std::max(n - 1, 1) + 255) / 256)) : INFINITY;
        TRUE(cost <= single * (1 + 1e-12));
        if (n > 1 && n < 9000) TRUE(cost >= prev * 0.999);          // longer filters never get cheaper
        if (n < 9000) prev = cost;
        TRUE(fir_history_len(n) == p.parts * p.ovl);                // what the slowest partition reaches back to
    }
    TRUE(plan(3841).parts == 2 && plan(3841).ovl == 2048);
    // beyond FIR_MAX_PARTS partitions of the largest overlap: no plan, and the direct kernel's history
    TRUE(plan(1024 * 3840).ok && !plan(1024 * 3840 + 1).ok && !plan(5000000).ok);
    TRUE(fir_history_len(5000000) == fir_single_overlap(5000000) && fir_single_overlap(5000000) == 5000192);
    TRUE(fir_history_len(1024 * 3840 + 1) == 1024 * 3840);
    // The tap counts one launch serves (the resampler builds its general-rate tables where plen + 1 is among them), as
    // found by running the planner over every count: 1 .. 2817, and 3073, the largest; none beyond.  Read against the
    // costs: 2817 taps need an overlap of 2816, 1 / 1280 a sample, where two partitions of 1536 cost 2.25 / 2560 = 1 / 1138;
    // 2818 .. 3072 need 3072, 1 / 1024, and lose to those two partitions; 3073 taps need two partitions of 1792, 2.25 / 2304
    // = 1 / 1024 exactly, a tie that the single launch, met first, keeps; from 3074 on a single launch costs 1 / 768 or more.
    for (int n = 1; n <= 20000; n++) TRUE((plan(n).parts == 1) == (n <= 2817 || n == 3073));
    TRUE(is(plan(2817), 2816, 1, 1280) && is(plan(2818), 1536, 2, 2560) && is(plan(3072), 1536, 2, 2560) && is(plan(3073), 3072, 1, 1024) &&
         is(plan(3074), 1792, 2, 2304));
}

static void test_size_class()
{
    TRUE(fir_size_class(0, 1) == 0 && fir_size_class(1, 1) == 0 && fir_size_class(2, 1) == 1 && fir_size_class(3, 1) == 1);
    for (int b = 2; b < 62; b++) {
        const long long v = 1LL << b;
        TRUE(fir_size_class(v - 1, 1) == b - 1 && fir_size_class(v, 1) == b && fir_size_class(v + 1, 1) == b);
    }
    // the channels count: 341 * 3 = 1023, 342 * 3 = 1026
    TRUE(fir_size_class(512, 2) == 10 && fir_size_class(511, 2) == 9 && fir_size_class(341, 3) == 9 && fir_size_class(342, 3) == 10);
    TRUE(fir_size_class(1LL << 40, 4) == 42 && fir_size_class(1, 64) == 6);
}

int main()
{
    const long double unit = -2.0L * acosl(-1.0L) / 4096;
    for (int q = 0; q < 4096; q++) {
        g_wr[q] = cosl(unit * q);
        g_wi[q] = sinl(unit * q);
    }
    // (taps, complex, sets, partitions, overlap); the last is the resampler's: three phases of 15 taps
    test_spectra(1, 0, 1, 1, 256);
    test_spectra(256, 0, 1, 1, 256);
    test_spectra(257, 1, 1, 1, 256);
    test_spectra(551, 1, 2, 1, 768);
    test_spectra(3841, 0, 1, 2, 2048);
    test_spectra(5000, 1, 3, 3, 1792);
    test_spectra(15, 0, 3, 1, 256);
    test_twiddles();
    test_planner();
    test_size_class();
    if (g_fails) {
        printf("fir plan: %d of %d FAILED\n", g_fails, g_checks);
        return 1;
    }
    printf("fir plan ok: %d checks; spectra within %.3f * 2^-24 of a partition's largest component\n", g_checks, g_worst);
    return 0;
}
