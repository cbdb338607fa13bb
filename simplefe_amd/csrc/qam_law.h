// qam_law.h -- the law of the QAM mapper and soft demapper (sfe_dsp_qam_*, include/sfe_dsp.h), operation by operation,
// compiled by qam.hip for the device, by api_qam.hip for sfe_dsp_qam_plan on the host, and by tests/host/test_qam_law.cpp
// with a plain host compiler.  Shared: the axis words and their odd integers, the level table, the place of a coded bit, the
// weight of a symbol, and the soft values of one axis -- twice: qam_axis_law is the statement, every word tried for every
// bit, and is what the host plan runs; qam_axis is what the kernel runs, the same e_v and the same minima found through
// partial minima that the bits share.  A minimum is exact, so the two give the same bits (test_qam_law.cpp holds them to
// it).  There is nothing here for a compiler to contract -- the one fused operation is an explicit fmaf -- and contraction
// is switched off in every function all the same.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define QAM_HD __host__ __device__
#else
#define QAM_HD
#endif

namespace sfe {

constexpr int QAM_MAX_AXIS_BITS = 4, QAM_MAX_WORDS = 16, QAM_MAX_BPS = 8;
constexpr int QAM_MAX_CSI_PERIOD = 4096, QAM_MAX_CSI_LEN = 65536;
constexpr size_t QAM_MAX_SYM = (size_t)1 << 24;

struct QamC {           // one cf32
    float r, i;
};

// bps of an order, 0 for an order the block does not have
QAM_HD inline int qam_bps(int order)
{
    return order == 2 ? 1 : order == 4 ? 2 : order == 16 ? 4 : order == 64 ? 6 : order == 256 ? 8 : 0;
}
QAM_HD inline int qam_axis_bits(int bps) { return bps == 1 ? 1 : bps / 2; }

// A(b_k ..) of the low `len` bits of w, the first of them the most significant: A() = 1, A(b, rest) = 2^(len(rest)+1) - (1 - 2b) A(rest)
inline int qam_A(unsigned w, int len)
{
    if (len == 0) return 1;
    const int b = (int)((w >> (len - 1)) & 1u);
    return (1 << len) - (1 - 2 * b) * qam_A(w, len - 1);
}
// the odd integer of the axis word w = (b_0 .. b_(m-1)), b_0 its most significant bit
inline int qam_u(unsigned w, int m) { return (1 - 2 * (int)((w >> (m - 1)) & 1u)) * qam_A(w, m - 1); }

// the integer K_M with d_M = 1 / sqrt(K_M): 1 for M = 2, else 2 (M - 1) / 3
inline int qam_K(int order) { return order == 2 ? 1 : 2 * (order - 1) / 3; }

// lev[w] = float32(amp u(w) / sqrt(K_M)), formed in float64 from the float32 amp and rounded once
inline void qam_levels(int order, float amp, float lev[QAM_MAX_WORDS])
{
    const int m = qam_axis_bits(qam_bps(order));
    const double root = sqrt((double)qam_K(order));
    for (int w = 0; w < QAM_MAX_WORDS; w++) lev[w] = w < (1 << m) ? (float)((double)amp * (double)qam_u((unsigned)w, m) / root) : 0.0f;
}

// coded bit v of a row of bytes: MSB-first
QAM_HD inline unsigned qam_coded_bit(const uint8_t *row, size_t v) { return ((unsigned)row[v >> 3] >> (7 - (unsigned)(v & 7))) & 1u; }

// ---- demap
// the weight of a symbol whose channel value is h
QAM_HD inline float qam_weight(QamC h, float scale)
{
#pragma clang fp contract(off)
    const float g = fmaf(h.i, h.i, h.r * h.r);
    return scale * g;
}

QAM_HD inline float qam_e(float y, float lev)
{
#pragma clang fp contract(off)
    const float t = y - lev;
    return t * t;
}

QAM_HD inline float qam_r(float w, float d0, float d1)
{
#pragma clang fp contract(off)
    const float d = d1 - d0;
    return w * d;
}

// The statement: r[c], c < m, of the axis value y under the weight w.  Every word for every bit.
QAM_HD inline void qam_axis_law(const float *lev, int m, float y, float w, float *r)
{
#pragma clang fp contract(off)
    for (int c = 0; c < m; c++) {
        float d0 = INFINITY, d1 = INFINITY;
        for (int v = 0; v < (1 << m); v++) {
            const float e = qam_e(y, lev[v]);
            if ((v >> (m - 1 - c)) & 1) d1 = fminf(d1, e);
            else d0 = fminf(d0, e);
        }
        r[c] = qam_r(w, d0, d1);
    }
}

// The same values with the minima shared between the bits.  A word is (hi, lo), HI = M - M / 2 bits over LO = M / 2 bits:
// ph[hi] is the minimum over lo and pl[lo] the minimum over hi, 2^M - 2^HI + 2^M - 2^LO minima in all; a bit of hi then
// needs the minimum of half of ph, a bit of lo of half of pl.  For M = 4 that is 32 minima where the statement has 56.
template <int M>
QAM_HD inline void qam_axis(const float *lev, float y, float w, float *r)
{
#pragma clang fp contract(off)
    constexpr int LO = M / 2, HI = M - LO, NH = 1 << HI, NL = 1 << LO;
    float e[1 << M], ph[NH], pl[NL];
#pragma unroll
    for (int v = 0; v < (1 << M); v++) e[v] = qam_e(y, lev[v]);
#pragma unroll
    for (int h = 0; h < NH; h++) {
        ph[h] = e[h << LO];
#pragma unroll
        for (int l = 1; l < NL; l++) ph[h] = fminf(ph[h], e[(h << LO) | l]);
    }
#pragma unroll
    for (int l = 0; l < NL; l++) {
        pl[l] = e[l];
#pragma unroll
        for (int h = 1; h < NH; h++) pl[l] = fminf(pl[l], e[(h << LO) | l]);
    }
#pragma unroll
    for (int c = 0; c < M; c++) {
        const bool in_hi = c < HI;
        const int n = in_hi ? NH : NL, bit = in_hi ? HI - 1 - c : M - 1 - c;
        const float *p = in_hi ? ph : pl;
        float d0 = INFINITY, d1 = INFINITY;
#pragma unroll
        for (int k = 0; k < n; k++) {
            if ((k >> bit) & 1) d1 = fminf(d1, p[k]);
            else d0 = fminf(d0, p[k]);
        }
        r[c] = qam_r(w, d0, d1);
    }
}

// the bps soft values of one symbol, in the order of its symbol-bit positions c = 0 .. bps - 1
template <int BPS>
QAM_HD inline void qam_symbol(const float *lev, QamC z, float w, float *r)
{
    constexpr int M = BPS == 1 ? 1 : BPS / 2;
    qam_axis<M>(lev, z.r, w, r);
    if (BPS > 1) qam_axis<M>(lev, z.i, w, r + M);
}

// ---- map: the two axis words of the bps bits of a symbol, its first bit the most significant of `bits`
QAM_HD inline QamC qam_point(const float *lev, int bps, unsigned bits)
{
    if (bps == 1) return QamC{lev[bits & 1u], 0.0f};
    const int m = bps / 2;
    return QamC{lev[(bits >> m) & ((1u << m) - 1u)], lev[bits & ((1u << m) - 1u)]};
}

}  // namespace sfe

// ---- the host's statement of a row (host functions: a device pass parses them and emits nothing)
namespace sfe {

struct QamShape {
    int order = 0, bps = 0, m = 0, csi_period = 0, csi_len = 0;
    size_t n_sym = 0;
    float scale = 0.0f;
    float lev[QAM_MAX_WORDS] = {};
    const uint32_t *perm = nullptr;         // [n_sym bps] or null
    const uint32_t *csi_index = nullptr;    // [csi_period]
};

// one row of coded bytes -> n_sym cf32 (any alignment: the words go out as bytes)
inline void qam_map_row_host(const QamShape &s, const uint8_t *row, unsigned char *out)
{
    for (size_t q = 0; q < s.n_sym; q++) {
        unsigned bits = 0;
        for (int c = 0; c < s.bps; c++) {
            const size_t t = q * (size_t)s.bps + (size_t)c;
            bits = (bits << 1) | qam_coded_bit(row, s.perm ? s.perm[t] : t);
        }
        const QamC p = qam_point(s.lev, s.bps, bits);
        __builtin_memcpy(out + 8 * q, &p, 8);
    }
}

// one row of n_sym cf32, and its csi row, -> n_sym bps floats
inline void qam_demap_row_host(const QamShape &s, const unsigned char *sym, const unsigned char *csi, unsigned char *out)
{
    for (size_t q = 0; q < s.n_sym; q++) {
        QamC z;
        __builtin_memcpy(&z, sym + 8 * q, 8);
        float w = s.scale;
        if (s.csi_period > 0) {
            QamC h;
            __builtin_memcpy(&h, csi + 8 * (size_t)s.csi_index[q % (size_t)s.csi_period], 8);
            w = qam_weight(h, s.scale);
        }
        float r[QAM_MAX_BPS];
        qam_axis_law(s.lev, s.m, z.r, w, r);
        if (s.bps > 1) qam_axis_law(s.lev, s.m, z.i, w, r + s.m);
        for (int c = 0; c < s.bps; c++) {
            const size_t t = q * (size_t)s.bps + (size_t)c;
            __builtin_memcpy(out + 4 * (size_t)(s.perm ? s.perm[t] : t), &r[c], 4);
        }
    }
}

}  // namespace sfe
