// ofdmmod_law.h -- the law of the OFDM burst modulator (sfe_dsp_ofdmmod_*, include/sfe_dsp.h), operation by operation,
// compiled by ofdmmod.hip for the device, by api_ofdmmod.hip for sfe_dsp_ofdmmod_plan on the host, and by
// tests/host/test_ofdmmod_law.cpp with a plain host compiler.  The first half is what the two sides share: the value of a
// bin, the complex product, a butterfly of a pass with its twiddle and its place, the last product with 1 / N, the frame
// sample's place in the transform and the wire format's group.  The second half is the host's serial statement of one
// symbol and of one frame.  There is nothing here for a compiler to contract: every multiply that feeds an add is an
// explicit fmaf, and every other product stands alone.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define OMOD_HD __host__ __device__
#else
#define OMOD_HD
#endif

namespace sfe {

constexpr int OMOD_MIN_LOGN = 6, OMOD_MAX_LOGN = 12, OMOD_MAX_TRAIN = 4, OMOD_MAX_DATA = 4096;
constexpr int OMOD_KIND_NULL = 0, OMOD_KIND_DATA = 1, OMOD_KIND_PILOT = 2;     // kind[k], as sfe_dsp_ofdm_*
constexpr int OMOD_SRC_NULL = -1, OMOD_SRC_PILOT = -2;                          // src[k]; a data bin holds its index i < Nd

struct alignas(8) omc {     // one cf32
    float x, y;
};

// A shape as both sides read it.  The tables are the handle's on the device and the plan's on the host.
struct OmodLaw {
    const omc *tw;          // [N]: exp(+j 2 pi q / N), from float64, rounded once (om_twiddles)
    const omc *ta;          // [N]: amp train on used bins, +0 on null bins
    const omc *pa;          // [N]: amp pilot on pilot bins, +0 elsewhere
    const float *sign;      // [Ns]: +-1
    const int *src;         // [N]: the bin list -- OMOD_SRC_NULL, OMOD_SRC_PILOT, or the data bin's index i in increasing k
    int logn, cp, T, Ns, Nd, order, symbols;        // symbols: SFE_OFDMMOD_IN_SYMBOLS
    float amp, a;           // a: a data symbol's component in BITS mode -- amp (order 2), float32(amp / sqrt 2) (order 4)
};

OMOD_HD inline omc om_add(omc a, omc b) { return omc{a.x + b.x, a.y + b.y}; }
OMOD_HD inline omc om_sub(omc a, omc b) { return omc{a.x - b.x, a.y - b.y}; }
OMOD_HD inline omc om_add_pj(omc a, omc b) { return omc{a.x - b.y, a.y + b.x}; }       // a + j b
OMOD_HD inline omc om_add_mj(omc a, omc b) { return omc{a.x + b.y, a.y - b.x}; }       // a - j b
// a b: two explicit fmaf, each over one rounded product (ofdm.hip: mul)
OMOD_HD inline omc om_mul(omc a, omc b) { return omc{fmaf(a.x, b.x, -(a.y * b.y)), fmaf(a.y, b.x, a.x * b.y)}; }

// ---- bins: X_j[k] of the burst whose input row is `row` (bytes in BITS mode, cf32 in SYMBOLS mode), j < T + Ns, k < N
OMOD_HD inline omc om_bin(const OmodLaw &L, const void *row, int j, int k)
{
    if (j < L.T) return L.ta[k];
    const int jd = j - L.T, s = L.src[k];
    if (s == OMOD_SRC_NULL) return omc{0.0f, 0.0f};
    if (s == OMOD_SRC_PILOT) {
        const float sg = L.sign[jd];
        return omc{L.pa[k].x * sg, L.pa[k].y * sg};
    }
    const int i = jd * L.Nd + s;
    if (L.symbols) {
        const omc v = static_cast<const omc *>(row)[i];
        return omc{v.x * L.amp, v.y * L.amp};
    }
    const uint8_t *bytes = static_cast<const uint8_t *>(row);
    if (L.order == 2) {
        const unsigned c = ((unsigned)bytes[i >> 3] >> (7 - (i & 7))) & 1u;
        return omc{c ? -L.a : L.a, 0.0f};
    }
    const int t = 2 * i;                                        // even: both bits lie in one byte
    const unsigned w = bytes[t >> 3], c0 = (w >> (7 - (t & 7))) & 1u, c1 = (w >> (6 - (t & 7))) & 1u;
    return omc{c0 ? -L.a : L.a, c1 ? -L.a : L.a};
}

// ---- transform: Stockham passes over N = 2^logn values, natural order in and out.  The pass that turns sub-transforms of
// length Ls = 2^logLs into ones of length R Ls has N / R butterflies; butterfly j reads in[j + r N / R], r < R, into x and
// leaves in x what goes to out[om_out_base<R>(logLs, j) + r Ls].  One radix-2 pass (logLs = 0) when logn is odd, then
// radix-4 passes.  A pass with logLs = 0 has no twiddles.
template <int R>
OMOD_HD inline int om_out_base(int logLs, int j)
{
    return ((j >> logLs) << (logLs + (R == 4 ? 2 : 1))) + (j & ((1 << logLs) - 1));
}

template <int R>
OMOD_HD inline void om_butterfly(int logn, int logLs, int j, const omc *tw, omc (&x)[R])
{
    constexpr int LOGR = R == 4 ? 2 : 1;
    if (logLs > 0) {
        const int k = j & ((1 << logLs) - 1);
        for (int r = 1; r < R; r++) x[r] = om_mul(x[r], tw[(r * k) << (logn - logLs - LOGR)]);
    }
    if constexpr (R == 4) {
        const omc t0 = om_add(x[0], x[2]), t1 = om_sub(x[0], x[2]), t2 = om_add(x[1], x[3]), t3 = om_sub(x[1], x[3]);
        x[0] = om_add(t0, t2);
        x[1] = om_add_pj(t1, t3);       // x0 + j x1 - x2 - j x3
        x[2] = om_sub(t0, t2);
        x[3] = om_add_mj(t1, t3);
    } else {
        const omc t0 = om_add(x[0], x[1]), t1 = om_sub(x[0], x[1]);
        x[0] = t0;
        x[1] = t1;
    }
}

// the last step: the product with the exact power of two 1 / N
OMOD_HD inline omc om_scale(omc v, float inv_n) { return omc{v.x * inv_n, v.y * inv_n}; }

// ---- frame: sample m < N + cp of a symbol is x[om_frame_src(m)] -- the tail x[N - cp .. N) as prefix, then x[0 .. N)
OMOD_HD inline int om_frame_src(int m, int N, int cp) { return (m + N - cp) & (N - 1); }

// ---- TX10: the quantiser of sfe_dsp_tx_f32_to_10bit (the device's conversion saturates; the host says so in words), and the
// group of two samples -- byte 0 in the low byte of w, byte 4 apart
OMOD_HD inline unsigned om_q10(float x)
{
    const float p = x * 511.0f;
#ifdef __HIP_DEVICE_COMPILE__
    const int v = (int)p;
#else
    int v;
    if (p != p) v = 0;
    else if (p >= 2147483648.0f) v = 2147483647;
    else if (p <= -2147483648.0f) v = -2147483647 - 1;
    else v = (int)p;
#endif
    return (unsigned)((int)(short)v + 512) & 0x3FFu;
}

OMOD_HD inline void om_group(omc y0, omc y1, uint32_t *w, uint8_t *last)
{
    const unsigned u0 = om_q10(y0.x), u1 = om_q10(y0.y), u2 = om_q10(y1.x), u3 = om_q10(y1.y);
    *w = ((u0 >> 8) | ((u1 >> 8) << 2) | ((u2 >> 8) << 4) | ((u3 >> 8) << 6)) | ((u0 & 0xFFu) << 8) | ((u1 & 0xFFu) << 16) | ((u2 & 0xFFu) << 24);
    *last = (uint8_t)u3;
}

}  // namespace sfe

// ---- the host's statement of the law (host functions: a device pass parses them and emits nothing)
namespace sfe {

// exp(+j 2 pi q / N), q < N, N a multiple of 4: cos and sin in float64, rounded once; the quarter turns exact
inline void om_twiddles(int N, omc *tw)
{
    const float cq[4] = {1.0f, 0.0f, -1.0f, 0.0f}, sq[4] = {0.0f, 1.0f, 0.0f, -1.0f};
    for (int q = 0; q < N; q++) {
        const double a = 2.0 * 3.14159265358979323846 * q / N;
        tw[q] = omc{(float)cos(a), (float)sin(a)};
        if (q % (N / 4) == 0) tw[q] = omc{cq[q / (N / 4)], sq[q / (N / 4)]};
    }
}

template <int R>
inline void om_pass_host(int logn, int logLs, const omc *tw, const omc *in, omc *out)
{
    const int NQ = (1 << logn) / R, Ls = 1 << logLs;
    for (int j = 0; j < NQ; j++) {
        omc x[R];
        for (int r = 0; r < R; r++) x[r] = in[j + r * NQ];
        om_butterfly<R>(logn, logLs, j, tw, x);
        const int base = om_out_base<R>(logLs, j);
        for (int r = 0; r < R; r++) out[base + r * Ls] = x[r];
    }
}

// v[0 .. N): X in, x = (1 / N) sum_k X[k] exp(+j 2 pi k n / N) out; tmp[0 .. N) is the passes' other buffer
inline void om_transform_host(int logn, const omc *tw, omc *v, omc *tmp)
{
    const int N = 1 << logn;
    omc *a = v, *b = tmp;
    int logLs = 0;
    if (logn & 1) {
        om_pass_host<2>(logn, 0, tw, a, b);
        omc *t = a;
        a = b, b = t;
        logLs = 1;
    }
    for (; logLs < logn; logLs += 2) {
        om_pass_host<4>(logn, logLs, tw, a, b);
        omc *t = a;
        a = b, b = t;
    }
    const float inv_n = 1.0f / (float)N;
    for (int n = 0; n < N; n++) v[n] = om_scale(a[n], inv_n);
}

// symbol j of one burst: N + cp samples into y; v and tmp are N values each
inline void om_symbol_host(const OmodLaw &L, const void *row, int j, omc *v, omc *tmp, omc *y)
{
    const int N = 1 << L.logn;
    for (int k = 0; k < N; k++) v[k] = om_bin(L, row, j, k);
    om_transform_host(L.logn, L.tw, v, tmp);
    for (int m = 0; m < N + L.cp; m++) y[m] = v[om_frame_src(m, N, L.cp)];
}

// the frame of one burst: F = (T + Ns)(N + cp) samples into y
inline void om_frame_host(const OmodLaw &L, const void *row, omc *v, omc *tmp, omc *y)
{
    const size_t len = ((size_t)1 << L.logn) + (size_t)L.cp;
    for (int j = 0; j < L.T + L.Ns; j++) om_symbol_host(L, row, j, v, tmp, y + (size_t)j * len);
}

// n samples (n even) as n / 2 groups of 5 bytes
inline void om_tx10_host(const omc *y, size_t n, uint8_t *o)
{
    for (size_t g = 0; g < n / 2; g++, o += 5) {
        uint32_t w;
        om_group(y[2 * g], y[2 * g + 1], &w, o + 4);
        o[0] = (uint8_t)w, o[1] = (uint8_t)(w >> 8), o[2] = (uint8_t)(w >> 16), o[3] = (uint8_t)(w >> 24);
    }
}

}  // namespace sfe
