// The QAM mapper and demapper's law (simplefe_amd/csrc/qam_law.h) on the host, for a build with
// -fsanitize=address,undefined (tests/test_qam_host.py builds and runs it).  A stand-alone program: it makes its own inputs
// from a fixed generator.  Every buffer is a heap block of exactly the size the contract names, so a store or a load one
// element outside is a report.
//   - the axis words: m = 2 stands at 11, 10, 00, 01 -> -3, -1, +1, +3; for every m the integers are the odd numbers of
//     [-(2^m - 1), 2^m - 1], each once, neighbours differ in one bit, b_0 = 0 is the positive half
//   - the kernel's form of an axis (qam_axis<M>, shared minima) gives the bits of the statement (qam_axis_law)
//   - a row through qam_map_row_host and qam_demap_row_host, with and without perm and csi, against a brute-force double
//     loop in float64 over all M points of the plane: |r - r_ref| <= 8 * 2^-24 * w * (D0 + D1), D0 and D1 the axis's own;
//     and the soft values of a mapped row have the signs of its bits, none of them zero, each at perm[t]
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../simplefe_amd/csrc/qam_law.h"

using namespace sfe;

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd()
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_state >> 32);
}
static double uni() { return ((double)rnd() + 0.5) / 4294967296.0; }            // (0, 1)
static double gauss() { return sqrt(-2.0 * log(uni())) * cos(6.283185307179586 * uni()); }

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

template <int M>
static void axis_kernel_form(const float *lev, float y, float w, float *r) { qam_axis<M>(lev, y, w, r); }

int main()
{
    long checks = 0;
    // ---- the axis words
    {
        const int want2[4] = {1, 3, -1, -3};
        for (unsigned w = 0; w < 4; w++) CHECK(qam_u(w, 2) == want2[w], "m = 2, word %u: %d", w, qam_u(w, 2));
        for (int m = 1; m <= QAM_MAX_AXIS_BITS; m++) {
            const int W = 1 << m;
            int *word_at = (int *)malloc((size_t)W * sizeof(int));     // by position (u + W - 1) / 2
            if (!word_at) return 3;
            for (int p = 0; p < W; p++) word_at[p] = -1;
            for (int w = 0; w < W; w++) {
                const int u = qam_u((unsigned)w, m);
                CHECK((u & 1) && u >= -(W - 1) && u <= W - 1, "m = %d, word %d: u = %d", m, w, u);
                CHECK(word_at[(u + W - 1) / 2] == -1, "m = %d: u = %d twice", m, u);
                word_at[(u + W - 1) / 2] = w;
                CHECK((u > 0) == !((w >> (m - 1)) & 1), "m = %d, word %d: b_0 = 0 is the positive half", m, w);
            }
            for (int p = 0; p + 1 < W; p++) CHECK(__builtin_popcount((unsigned)(word_at[p] ^ word_at[p + 1])) == 1, "m = %d: positions %d, %d", m, p, p + 1);
            free(word_at);
        }
    }
    const int orders[5] = {2, 4, 16, 64, 256};
    double worst_ratio = 0.0;
    // ---- an axis: the kernel's form against the statement, and the statement against float64
    for (int oi = 0; oi < 5; oi++) {
        const int order = orders[oi], bps = qam_bps(order), m = qam_axis_bits(bps), W = 1 << m;
        for (int si = 0; si < 3; si++) {
            const float amp = si == 0 ? 1.0f : si == 1 ? 3.7e-6f : 2.9e5f;
            float *lev = (float *)malloc((size_t)QAM_MAX_WORDS * sizeof(float));
            if (!lev) return 3;
            qam_levels(order, amp, lev);
            const double step = 2.0 * (double)amp / sqrt((double)qam_K(order));
            for (int n = 0; n < 4000; n++) {
                const int v = (int)(rnd() % (unsigned)W);
                const double noise = n % 4 == 0 ? 0.02 : n % 4 == 1 ? 0.3 : n % 4 == 2 ? 1.0 : 5.0;
                const float y = (float)((double)lev[v] + noise * step * gauss());
                const float w = (float)(0.01 + 3.0 * uni());
                float *a = (float *)malloc((size_t)m * sizeof(float)), *b = (float *)malloc((size_t)m * sizeof(float));
                if (!a || !b) return 3;
                qam_axis_law(lev, m, y, w, a);
                if (m == 1) axis_kernel_form<1>(lev, y, w, b);
                if (m == 2) axis_kernel_form<2>(lev, y, w, b);
                if (m == 3) axis_kernel_form<3>(lev, y, w, b);
                if (m == 4) axis_kernel_form<4>(lev, y, w, b);
                CHECK(memcmp(a, b, (size_t)m * sizeof(float)) == 0, "order %d, y = %a: the two forms differ", order, y);
                for (int c = 0; c < m; c++) {
                    double d0 = INFINITY, d1 = INFINITY;
                    for (int u = 0; u < W; u++) {
                        const double t = (double)y - (double)lev[u], e = t * t;
                        if ((u >> (m - 1 - c)) & 1) d1 = fmin(d1, e);
                        else d0 = fmin(d0, e);
                    }
                    const double ref = (double)w * (d1 - d0), bar = 8.0 * ldexp(1.0, -24) * (double)w * (d0 + d1);
                    const double err = fabs((double)a[c] - ref);
                    if (bar > 0 && err / bar > worst_ratio) worst_ratio = err / bar;
                    CHECK(err <= bar, "order %d, y = %a, bit %d: |r - ref| = %g above %g", order, y, c, err, bar);
                }
                free(a);
                free(b);
            }
            free(lev);
        }
    }
    // ---- rows
    for (int oi = 0; oi < 5; oi++) {
        for (int variant = 0; variant < 4; variant++) {
            const int order = orders[oi], bps = qam_bps(order), m = qam_axis_bits(bps);
            const bool with_perm = variant & 1, with_csi = variant & 2;
            const size_t n_sym = 37 + (size_t)oi, B = n_sym * (size_t)bps, nbytes = (B + 7) / 8;
            const int period = 5, csi_len = 9;
            QamShape s;
            s.order = order, s.bps = bps, s.m = m, s.n_sym = n_sym, s.scale = 1.0f;
            s.csi_period = with_csi ? period : 0, s.csi_len = with_csi ? csi_len : 0;
            qam_levels(order, 0.8f, s.lev);
            uint32_t *perm = (uint32_t *)malloc(B * sizeof(uint32_t)), *idx = (uint32_t *)malloc((size_t)period * sizeof(uint32_t));
            uint8_t *bytes = (uint8_t *)malloc(nbytes);
            unsigned char *sym = (unsigned char *)malloc(n_sym * 8), *csi = (unsigned char *)malloc((size_t)csi_len * 8);
            unsigned char *soft = (unsigned char *)malloc(B * 4);
            if (!perm || !idx || !bytes || !sym || !csi || !soft) return 3;
            for (size_t t = 0; t < B; t++) perm[t] = (uint32_t)t;
            for (size_t t = B - 1; t > 0; t--) {
                const size_t j = rnd() % (t + 1);
                const uint32_t x = perm[t];
                perm[t] = perm[j], perm[j] = x;
            }
            for (int i = 0; i < period; i++) idx[i] = rnd() % (unsigned)csi_len;
            for (size_t i = 0; i < nbytes; i++) bytes[i] = (uint8_t)rnd();
            for (int i = 0; i < csi_len; i++) {
                const QamC h{(float)(0.3 + uni()), (float)(uni() - 0.5)};
                memcpy(csi + 8 * i, &h, 8);
            }
            s.perm = with_perm ? perm : nullptr;
            s.csi_index = with_csi ? idx : nullptr;
            qam_map_row_host(s, bytes, sym);
            memset(soft, 0xA5, B * 4);
            qam_demap_row_host(s, sym, with_csi ? csi : nullptr, soft);
            // the soft values of a mapped row: the signs of its bits, none zero, each at perm[t]; and against float64 over the plane
            const int W = 1 << m, M = order;
            for (size_t q = 0; q < n_sym; q++) {
                QamC z;
                memcpy(&z, sym + 8 * q, 8);
                double w = 1.0;
                if (with_csi) {
                    QamC h;
                    memcpy(&h, csi + 8 * idx[q % (size_t)period], 8);
                    w = (double)h.r * h.r + (double)h.i * h.i;
                }
                for (int c = 0; c < bps; c++) {
                    const size_t t = q * (size_t)bps + (size_t)c, v = with_perm ? perm[t] : t;
                    float r;
                    memcpy(&r, soft + 4 * v, 4);
                    const unsigned bit = qam_coded_bit(bytes, v);
                    CHECK(r != 0.0f && (r < 0.0f) == (bit == 1), "order %d, variant %d, symbol %zu, bit %d: r = %g for bit %u", order, variant, q, c, r, bit);
                    double d0 = INFINITY, d1 = INFINITY, a0 = INFINITY, a1 = INFINITY;
                    for (int p = 0; p < M; p++) {           // every point of the plane: its words, its bit c
                        const int wi = bps == 1 ? p : p >> m, wq = bps == 1 ? 0 : p & (W - 1);
                        const double di = (double)z.r - (double)s.lev[wi], dq = bps == 1 ? 0.0 : (double)z.i - (double)s.lev[wq];
                        const double e = di * di + dq * dq;
                        const int pb = c < m ? (wi >> (m - 1 - c)) & 1 : (wq >> (m - 1 - (c - m))) & 1;
                        if (pb) d1 = fmin(d1, e);
                        else d0 = fmin(d0, e);
                    }
                    for (int u = 0; u < W; u++) {           // the axis's own D0 and D1, for the bar
                        const double y = c < m ? z.r : z.i, tt = y - (double)s.lev[u], e = tt * tt;
                        if ((u >> (m - 1 - (c < m ? c : c - m))) & 1) a1 = fmin(a1, e);
                        else a0 = fmin(a0, e);
                    }
                    const double ref = w * (d1 - d0), bar = 8.0 * ldexp(1.0, -24) * w * (a0 + a1), err = fabs((double)r - ref);
                    if (bar > 0 && err / bar > worst_ratio) worst_ratio = err / bar;
                    CHECK(err <= bar, "order %d, variant %d, symbol %zu, bit %d: |r - ref| = %g above %g", order, variant, q, c, err, bar);
                }
            }
            free(perm), free(idx), free(bytes), free(sym), free(csi), free(soft);
        }
    }
    // ---- the exact case
    {
        float lev[QAM_MAX_WORDS], r[1];
        qam_levels(2, 1.0f, lev);
        CHECK(lev[0] == 1.0f && lev[1] == -1.0f, "order 2 levels %g %g", lev[0], lev[1]);
        qam_axis_law(lev, 1, 0.5f, 1.0f, r);
        CHECK(r[0] == 2.0f, "the exact case gives %g", r[0]);
    }
    printf("qam law ok: %ld checks, worst |r - ref| / bar %.3f\n", checks, worst_ratio);
    return 0;
}
