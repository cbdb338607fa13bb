// fsk_law.h -- the law of the 2-(G)FSK burst modem (sfe_dsp_fsk_*, include/sfe_dsp.h), operation by operation, compiled by
// fsk.hip for the device, by api_fsk.hip for sfe_dsp_fsk_plan on the host, and by tests/host/test_fsk_law.cpp with a plain
// host compiler.  Shared: the integer phase of a frame (the level sum of the symbols whose pulse has passed, times Gsum, plus
// the at most Q symbols in flight), fsk_cis, the pairwise tree, and the steps of the fit.  The discriminator is
// polar_law.h's polar_sample<POLAR_FM>, included here and not copied; that header needs the HIP compiler, so the filter chain
// fsk_u is compiled by the two HIP sides only.  Every multiply that feeds an add is an explicit fmaf, everything else is one
// IEEE float32 operation or exact integer arithmetic mod 2^32, and contraction is switched off in every function that
// computes all the same.
//
// M = 2 ONLY.  4-level FSK is not built: a float64 probe of this symbol-by-symbol slicer at BT = 0.5 made 95 errors in 2560
// bits at 26 dB -- the inter-symbol interference of the inner levels needs a sequence detector.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

#include "polar_law.h"
#define FSK_HD __host__ __device__
#else
#define FSK_HD
#endif

namespace sfe {

constexpr int FSK_MIN_SPS = 2, FSK_MAX_SPS = 64, FSK_MAX_ARM = 64;         // samples per symbol; symbols a pulse spans (Q)
constexpr int FSK_MAX_TAPS = FSK_MAX_ARM * FSK_MAX_SPS;
constexpr int FSK_MAX_PRE = 1024, FSK_MAX_BITS = 32768, FSK_MAX_MF = 256, FSK_MAX_DELAY = 1 << 20, FSK_MAX_RANGE = 64;
constexpr int FSK_OK = 0, FSK_NO_ESTIMATE = 1, FSK_GATED = 2, FSK_OUT_OF_RANGE = 3;
constexpr int FSK_REC = 8;              // float32 words of a record: tau, f, dev, q, +0, +0, +0, +0

// sin(pi t / 4) / t and (cos(pi t / 4) - 1) / t^2 as cubics in z = t^2 on [0, 1]: least-squares fits at 64 Chebyshev nodes
// in z, formed in float64 and rounded once
constexpr float FSK_S0 = 0x1.921fb6p-1f, FSK_S1 = -0x1.4abbbap-4f, FSK_S2 = 0x1.465ec4p-9f, FSK_S3 = -0x1.2d9b7cp-15f;
constexpr float FSK_C0 = -0x1.3bd3ccp-2f, FSK_C1 = 0x1.03c1eap-6f, FSK_C2 = -0x1.55cb98p-12f, FSK_C3 = 0x1.db64d2p-19f;
constexpr float FSK_INV_2PI = 0x1.45f306p-3f;

struct FskC {           // one cf32
    float r, i;
};

// (cos, sin) of the phase p / 2^32 turns.  The quadrant is exact; the remainder is at most an eighth of a turn either way.
FSK_HD inline FskC fsk_cis(uint32_t p)
{
#pragma clang fp contract(off)
    const uint32_t q = ((p + (1u << 29)) >> 30) & 3u;
    const int32_t r = (int32_t)(p - (q << 30));             // in [-2^29, 2^29)
    const float t = (float)r * 0x1p-29f, z = t * t;
    float sp = FSK_S3;
    sp = fmaf(sp, z, FSK_S2);
    sp = fmaf(sp, z, FSK_S1);
    sp = fmaf(sp, z, FSK_S0);
    const float s = t * sp;
    float c = FSK_C3;
    c = fmaf(c, z, FSK_C2);
    c = fmaf(c, z, FSK_C1);
    c = fmaf(c, z, FSK_C0);
    c = fmaf(c, z, 1.0f);
    if (q == 0) return FskC{c, s};
    if (q == 1) return FskC{-s, c};
    if (q == 2) return FskC{-c, -s};
    return FskC{s, -c};
}

// bit t of a row of bytes, MSB-first
FSK_HD inline unsigned fsk_bit(const uint8_t *row, int t) { return ((unsigned)row[t >> 3] >> (7 - (t & 7))) & 1u; }

// ones among the first n bits of a row, MSB-first (the statement; the kernel counts the same bits a byte per lane)
inline int fsk_ones(const uint8_t *row, int n)
{
    int c = 0;
    for (int t = 0; t < n; t++) c += (int)fsk_bit(row, t);
    return c;
}

// the symbols of a frame of N whose whole pulse lies before sample i: each contributes a_k Gsum to P[i]
FSK_HD inline int fsk_passed(int i, int sps, int n_taps, int N)
{
    if (i < n_taps) return 0;
    const int kp = (i - n_taps) / sps + 1;
    return kp < N ? kp : N;
}

// P[i] in its tile form: A is the sum of the levels of the kp = fsk_passed(i) symbols before kp, lev(k) = +1 or -1 the level
// of symbol k; the symbols kp .. min(i / sps, N - 1) are in flight, at most Q of them.  uint32 arithmetic, exact mod 2^32.
template <class Lev>
FSK_HD inline uint32_t fsk_phase(int i, int sps, int N, uint32_t Gsum, int A, int kp, const uint32_t *C, Lev lev)
{
    uint32_t p = Gsum * (uint32_t)A;
    int k1 = i / sps;
    if (k1 > N - 1) k1 = N - 1;
    for (int k = kp; k <= k1; k++) {
        const uint32_t c = C[i - k * sps];
        p += lev(k) > 0 ? c : 0u - c;
    }
    return p;
}

// one sample of the frame from its phase
FSK_HD inline FskC fsk_mod_sample(uint32_t p, float amp)
{
#pragma clang fp contract(off)
    const FskC e = fsk_cis(p);
    return FskC{amp * e.r, amp * e.i};
}

// ---- the pairwise tree over s[0 .. n2), n2 a power of two, padded with +0 by the caller: at each level s[k] = s[2k] + s[2k+1].
// In place, in the stride form: at the level of stride h, s[2hk] += s[2hk + h] -- the same additions in the same order, and
// the form the kernel runs with a barrier per level.  The sum is left in s[0].
FSK_HD inline int fsk_pow2(int n)
{
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}
inline float fsk_tree(float *s, int n2)
{
#pragma clang fp contract(off)
    for (int h = 1; h < n2; h <<= 1)
        for (int k = 0; k + h < n2; k += 2 * h) s[k] = s[k] + s[k + h];
    return s[0];
}

// ---- the fit of one timing candidate, and what follows from the best one
FSK_HD inline float fsk_num(int Lp, float Se, float se, float S1)
{
#pragma clang fp contract(off)
    const float t = se * S1;
    return fmaf((float)Lp, Se, -t);
}
struct FskFit {
    float dev, dc, f;
};
FSK_HD inline FskFit fsk_fit(int Lp, float num, float den, float se, float S1)
{
#pragma clang fp contract(off)
    FskFit r;
    r.dev = num / den;
    const float t = r.dev * se;
    r.dc = (S1 - t) / (float)Lp;
    r.f = r.dc * FSK_INV_2PI;
    return r;
}
FSK_HD inline bool fsk_fit_ok(float dev) { return dev > 0.0f && dev <= 3.402823466e+38f; }
FSK_HD inline float fsk_resid_term(float u, float e, float dev, float dc)
{
#pragma clang fp contract(off)
    const float d = u - fmaf(dev, e, dc);
    return d * d;
}
FSK_HD inline float fsk_quality(float resid, float dev, float see)
{
#pragma clang fp contract(off)
    const float d2 = dev * dev;
    return resid / (d2 * see);
}
FSK_HD inline float fsk_soft(float u, float dc, float dev, float scale)
{
#pragma clang fp contract(off)
    const float w = (u - dc) / dev;
    return scale * w;
}

#ifdef __HIPCC__
// u(i) = sum over j < n_mf of m[j] v[i + j], an fmaf chain from +0 in increasing j; v[n] = polar_sample<POLAR_FM>(x[n],
// x[n - 1], 1).  at(n) returns sample n of the burst's window as a PolarC.
template <class At>
FSK_HD inline float fsk_u(long long i, int n_mf, const float *m, At at)
{
#pragma clang fp contract(off)
    float acc = 0.0f;
    PolarC prev = at(i - 1);
    for (int j = 0; j < n_mf; j++) {
        const PolarC cur = at(i + j);
        acc = fmaf(m[j], polar_sample<POLAR_FM>(cur, prev, 1.0f), acc);
        prev = cur;
    }
    return acc;
}
#endif

}  // namespace sfe
