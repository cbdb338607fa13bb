// ldpc_law.h -- the law of the quasi-cyclic LDPC code (sfe_dsp_ldpc_*, include/sfe_dsp.h), compiled by ldpc.hip for the
// device, by api_ldpc.hip for sfe_dsp_ldpc_plan on the host, and by tests/host/test_ldpc_law.cpp with a plain host compiler.
// What the two sides share is the first half: the limits, the quantiser, and the update of one check row -- the same
// integer operations on the same int16 sums and int8 messages, so the device's bytes are the plan's.  The second half is
// the host's: the checker that turns a base matrix into a cell table, the serial decoder, and the encoder (the law names
// no algorithm for it: the codeword is unique where the parity part is invertible, so the kernel's word-parallel form and
// the serial one here agree by theorem).  Integer arithmetic apart from ONE float32 multiply and rintf in the quantiser.
//
// THE BOUND.  Nothing but a message's magnitude saturates.  APP[v] always equals L_v plus the current messages of v's
// checks, each of magnitude <= 127, and a variable sits in at most mb checks (one circulant per cell): |APP| <= 127 (1 + mb)
// <= 8255, and |Q| = |APP - R| <= 8382.  Both fit int16.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define LDPC_HD __host__ __device__
#else
#define LDPC_HD
#endif

namespace sfe {

constexpr int LDPC_MAX_Z = 512, LDPC_MAX_MB = 64, LDPC_MAX_NB = 256, LDPC_MAX_N = 8192, LDPC_MIN_DEG = 2, LDPC_MAX_DEG = 32;
constexpr int LDPC_MAX_EDGES = 65536, LDPC_MAX_CELLS = LDPC_MAX_MB * LDPC_MAX_DEG;
constexpr int LDPC_MAX_A = 16, LDPC_MAX_BETA = 127, LDPC_MAX_ITER = 64, LDPC_SAT = 127;
constexpr int LDPC_OK = 0, LDPC_NOT_FINITE = 1, LDPC_UPSTREAM = 2, LDPC_NOT_CONVERGED = 3;
static_assert(LDPC_SAT * (1 + LDPC_MAX_MB) + LDPC_SAT <= INT16_MAX, "APP and Q must fit int16");
static_assert(LDPC_MAX_EDGES <= 65536 && LDPC_MAX_N * 2 <= 65536, "edge and variable indices fit 16 bits and a word's LDS is bounded");

struct LdpcCell {
    uint16_t col, shift;        // block column, and the circulant's shift in [0, Z)
};

// L = clamp(rintf(r * scale), -127, 127): one IEEE multiply, ties to even; a product of +-inf clamps.  r is finite.
LDPC_HD inline int ldpc_quant(float r, float scale)
{
#ifdef __HIP_DEVICE_COMPILE__
    float p = rintf(__fmul_rn(r, scale));
#else
    volatile float prod = r * scale;        // kept a float32 product whatever the host compiler's excess precision
    float p = rintf(prod);
#endif
    p = p < -(float)LDPC_SAT ? -(float)LDPC_SAT : p;
    p = p > (float)LDPC_SAT ? (float)LDPC_SAT : p;
    return (int)p;
}

// M' = min(max(((M a) >> 4) - beta, 0), 127)
LDPC_HD inline int ldpc_mag(int M, int a, int beta)
{
    int v = ((M * a) >> 4) - beta;
    v = v < 0 ? 0 : v;
    return v > LDPC_SAT ? LDPC_SAT : v;
}

LDPC_HD inline int ldpc_var(LdpcCell c, int Z, int i)      // the variable of cell c in row i of its layer
{
    int x = i + (int)c.shift;
    x -= x >= Z ? Z : 0;
    return (int)c.col * Z + x;
}

// One check row: row i of the layer whose cells are cells[first .. first + d), in increasing block column.  app: the n
// sums; msg: one message per edge, edge (cell q, row i) at q Z + i.  Two passes over the cells, so that nothing of the row
// is kept but four scalars: the second pass forms Q_j again from values the first did not change.
LDPC_HD inline void ldpc_row_update(int16_t *app, int8_t *msg, const LdpcCell *cells, int first, int d, int Z, int i, int a, int beta)
{
    int m1 = 1 << 20, m2 = 1 << 20, js = 0;
    unsigned S = 0;
    for (int j = 0; j < d; j++) {
        const int Q = (int)app[ldpc_var(cells[first + j], Z, i)] - (int)msg[(first + j) * Z + i];
        const unsigned neg = Q < 0;
        const int mag = neg ? -Q : Q;
        S ^= neg;
        if (mag < m1) m2 = m1, m1 = mag, js = j;       // the lowest j attaining the minimum
        else if (mag < m2) m2 = mag;
    }
    const int M1 = ldpc_mag(m1, a, beta), M2 = ldpc_mag(m2, a, beta);
    for (int j = 0; j < d; j++) {
        const int v = ldpc_var(cells[first + j], Z, i), e = (first + j) * Z + i;
        const int Q = (int)app[v] - (int)msg[e];
        const int Mp = j == js ? M2 : M1;
        const int Rn = (S ^ (unsigned)(Q < 0)) ? -Mp : Mp;
        app[v] = (int16_t)(Q + Rn);
        msg[e] = (int8_t)Rn;
    }
}

// 1 iff the check of row i of that layer is unsatisfied by the decisions x_v = (APP[v] < 0)
LDPC_HD inline unsigned ldpc_row_parity(const int16_t *app, const LdpcCell *cells, int first, int d, int Z, int i)
{
    unsigned S = 0;
    for (int j = 0; j < d; j++) S ^= (unsigned)(app[ldpc_var(cells[first + j], Z, i)] < 0);
    return S;
}

}  // namespace sfe

// ------------------------------------------------------------------------------------------------ the host's half
#include <utility>
#include <vector>

namespace sfe {

// A validated code.  cells: every non-empty cell, block row after block row, in increasing block column; row r's are
// cells[row_start[r] .. row_start[r + 1]).  The encoder's table (ldpc_build_encoder) is empty where the code is not encodable.
struct LdpcCode {
    int mb = 0, nb = 0, Z = 0, n = 0, m = 0, k = 0, kb = 0, max_col_deg = 0;
    std::vector<LdpcCell> cells;
    std::vector<uint16_t> row_start;
    int encodable = 0, Zw = 0;
    // inv[(r mb + c) Zw + w]: bit j of the Z-bit sequence q_{r,c}[j] = Binv[r Z + j][c Z], 32 to a word, bit j & 31 of word
    // j >> 5; B is the parity part of H (its last m columns), and its inverse is block-circulant as B is
    std::vector<uint32_t> inv;
    int n_bytes() const { return (n + 7) / 8; }
    int k_bytes() const { return (k + 7) / 8; }
    size_t edges() const { return cells.size() * (size_t)Z; }
};

// 0 and *c filled in (without the encoder's table), or -1 and a message
inline int ldpc_check(int mb, int nb, int Z, const int16_t *shift, LdpcCode *c, char *msg, size_t cap)
{
    if (Z < 1 || Z > LDPC_MAX_Z) return snprintf(msg, cap, "Z = %d must be in [1, %d]", Z, LDPC_MAX_Z), -1;
    if (mb < 1 || mb > LDPC_MAX_MB) return snprintf(msg, cap, "mb = %d must be in [1, %d]", mb, LDPC_MAX_MB), -1;
    if (nb <= mb || nb > LDPC_MAX_NB) return snprintf(msg, cap, "nb = %d must be in (mb = %d, %d]", nb, mb, LDPC_MAX_NB), -1;
    if ((long long)nb * Z > LDPC_MAX_N) return snprintf(msg, cap, "n = nb Z = %lld must be at most %d", (long long)nb * Z, LDPC_MAX_N), -1;
    if (!shift) return snprintf(msg, cap, "null base matrix"), -1;
    LdpcCode o;
    o.mb = mb, o.nb = nb, o.Z = Z, o.n = nb * Z, o.m = mb * Z, o.k = o.n - o.m, o.kb = nb - mb;
    std::vector<int> coldeg(nb, 0);
    o.row_start.push_back(0);
    for (int r = 0; r < mb; r++) {
        int d = 0;
        for (int col = 0; col < nb; col++) {
            const int s = shift[(size_t)r * nb + col];
            if (s == -1) continue;
            if (s < 0 || s >= Z) return snprintf(msg, cap, "shift[%d][%d] = %d must be -1 (empty) or in [0, Z = %d)", r, col, s, Z), -1;
            o.cells.push_back(LdpcCell{(uint16_t)col, (uint16_t)s});
            d++, coldeg[col]++;
        }
        if (d < LDPC_MIN_DEG || d > LDPC_MAX_DEG)
            return snprintf(msg, cap, "block row %d has %d cells: must be in [%d, %d]", r, d, LDPC_MIN_DEG, LDPC_MAX_DEG), -1;
        o.row_start.push_back((uint16_t)o.cells.size());
    }
    for (int col = 0; col < nb; col++) {
        if (coldeg[col] == 0) return snprintf(msg, cap, "block column %d has no cell", col), -1;
        if (coldeg[col] > o.max_col_deg) o.max_col_deg = coldeg[col];
    }
    if (o.edges() > (size_t)LDPC_MAX_EDGES)
        return snprintf(msg, cap, "cells Z = %zu edges: at most %d", o.edges(), LDPC_MAX_EDGES), -1;
    *c = std::move(o);
    return 0;
}

inline int ldpc_check_params(float scale, int a, int beta, int max_iter, char *msg, size_t cap)
{
    if (!(scale > 0.0f) || !(fabsf(scale) <= 3.4028234663852886e38f)) return snprintf(msg, cap, "scale = %g must be finite and > 0", (double)scale), -1;
    if (a < 1 || a > LDPC_MAX_A) return snprintf(msg, cap, "a = %d must be in [1, %d]", a, LDPC_MAX_A), -1;
    if (beta < 0 || beta > LDPC_MAX_BETA) return snprintf(msg, cap, "beta = %d must be in [0, %d]", beta, LDPC_MAX_BETA), -1;
    if (max_iter < 1 || max_iter > LDPC_MAX_ITER) return snprintf(msg, cap, "max_iter = %d must be in [1, %d]", max_iter, LDPC_MAX_ITER), -1;
    return 0;
}

// Is the parity part B (the last m columns of H) invertible over GF(2), and if so its inverse's block columns: dense
// Gauss-Jordan on [B | e_0, e_Z, e_2Z ...], rows of 64-bit words.  B^-1 is block-circulant, so its columns c Z are all of it.
inline void ldpc_build_encoder(LdpcCode *c)
{
    const int m = c->m, mb = c->mb, Z = c->Z, kb = c->kb;
    const int W = (m + mb + 63) / 64;
    std::vector<uint64_t> M((size_t)m * W, 0);
    auto flip = [&](int row, int col) { M[(size_t)row * W + (col >> 6)] ^= 1ull << (col & 63); };
    for (int r = 0; r < mb; r++)
        for (int q = c->row_start[r]; q < c->row_start[r + 1]; q++) {
            const LdpcCell ce = c->cells[q];
            if ((int)ce.col < kb) continue;
            for (int i = 0; i < Z; i++) flip(r * Z + i, ldpc_var(ce, Z, i) - c->k);
        }
    for (int b = 0; b < mb; b++) flip(b * Z, m + b);
    c->encodable = 0, c->Zw = (Z + 31) / 32;
    c->inv.clear();
    for (int p = 0; p < m; p++) {
        const int w0 = p >> 6;
        const uint64_t bit = 1ull << (p & 63);
        int piv = -1;
        for (int r = p; r < m; r++)
            if (M[(size_t)r * W + w0] & bit) {
                piv = r;
                break;
            }
        if (piv < 0) return;                            // singular
        if (piv != p)
            for (int w = 0; w < W; w++) std::swap(M[(size_t)p * W + w], M[(size_t)piv * W + w]);
        const uint64_t *src = &M[(size_t)p * W];
        for (int r = 0; r < m; r++) {
            if (r == p || !(M[(size_t)r * W + w0] & bit)) continue;
            uint64_t *dst = &M[(size_t)r * W];
            for (int w = w0; w < W; w++) dst[w] ^= src[w];      // the pivot row is zero in front of its pivot
        }
    }
    c->encodable = 1;
    c->inv.assign((size_t)mb * mb * c->Zw, 0u);
    for (int r = 0; r < mb; r++)
        for (int b = 0; b < mb; b++)
            for (int j = 0; j < Z; j++)
                if ((M[(size_t)(r * Z + j) * W + ((m + b) >> 6)] >> ((m + b) & 63)) & 1ull) c->inv[((size_t)r * mb + b) * c->Zw + (j >> 5)] |= 1u << (j & 31);
}

inline int ldpc_get_bit(const uint8_t *bytes, int g) { return (bytes[g >> 3] >> (7 - (g & 7))) & 1; }

// One codeword of an encodable code: c[0 .. k) = the payload's bits, H c = 0.  s = A u over the information part, then
// p = B^-1 s: column c Z + t of B^-1 is column c Z rotated down by t within every block.  out: ceil(n / 8) bytes, pad bits 0.
inline void ldpc_encode_word(const LdpcCode &c, const uint8_t *payload, uint8_t *out)
{
    const int Z = c.Z, mb = c.mb, k = c.k;
    std::vector<uint8_t> s((size_t)c.m, 0), p((size_t)c.m, 0), qq((size_t)2 * Z);
    for (int r = 0; r < mb; r++)
        for (int q = c.row_start[r]; q < c.row_start[r + 1]; q++) {
            const LdpcCell ce = c.cells[q];
            if ((int)ce.col >= c.kb) continue;
            for (int i = 0; i < Z; i++) s[(size_t)r * Z + i] ^= (uint8_t)ldpc_get_bit(payload, ldpc_var(ce, Z, i));
        }
    for (int r = 0; r < mb; r++)
        for (int b = 0; b < mb; b++) {
            const uint32_t *w = &c.inv[((size_t)r * mb + b) * c.Zw];
            bool any = false;
            for (int j = 0; j < Z; j++) any |= (qq[j] = qq[j + Z] = (uint8_t)((w[j >> 5] >> (j & 31)) & 1u)) != 0;
            if (!any) continue;
            for (int t = 0; t < Z; t++) {
                if (!s[(size_t)b * Z + t]) continue;
                const uint8_t *rot = &qq[Z - t];        // rot[i] = q[(i - t) mod Z]
                uint8_t *dst = &p[(size_t)r * Z];
                for (int i = 0; i < Z; i++) dst[i] ^= rot[i];
            }
        }
    memset(out, 0, (size_t)c.n_bytes());
    for (int g = 0; g < k; g++) out[g >> 3] |= (uint8_t)(ldpc_get_bit(payload, g) << (7 - (g & 7)));
    for (int g = 0; g < c.m; g++) out[(k + g) >> 3] |= (uint8_t)(p[g] << (7 - ((k + g) & 7)));
}

// Scratch of the serial decoder, made once per plan call.
struct LdpcWork {
    std::vector<int16_t> app;
    std::vector<int8_t> msg, L;
};

// what a word without an answer gets; each output may be null
inline void ldpc_fail_word(const LdpcCode &c, int st, uint8_t *bytes, uint32_t *rec, int *status)
{
    if (bytes) memset(bytes, 0, (size_t)c.k_bytes());
    if (rec) rec[0] = rec[1] = rec[2] = 0u;
    if (status) *status = st;
}

inline unsigned ldpc_unsatisfied(const LdpcCode &c, const int16_t *app)
{
    unsigned u = 0;
    for (int r = 0; r < c.mb; r++)
        for (int i = 0; i < c.Z; i++) u += ldpc_row_parity(app, c.cells.data(), c.row_start[r], c.row_start[r + 1] - c.row_start[r], c.Z, i);
    return u;
}

// The law on one codeword: soft value v is row[v mul].  Returns the largest |APP| met (for the bound's test).
inline int ldpc_decode_word(const LdpcCode &c, LdpcWork &w, const float *row, int mul, float scale, int a, int beta, int max_iter, uint8_t *bytes,
                            uint32_t *rec, int *status)
{
    const int n = c.n, Z = c.Z;
    for (int v = 0; v < n; v++)
        if (!(fabsf(row[(size_t)v * mul]) <= 3.4028234663852886e38f)) return ldpc_fail_word(c, LDPC_NOT_FINITE, bytes, rec, status), 0;
    w.app.resize(n), w.L.resize(n);
    w.msg.assign(c.edges(), 0);
    for (int v = 0; v < n; v++) w.app[v] = w.L[v] = (int8_t)ldpc_quant(row[(size_t)v * mul], scale);
    int peak = 0;
    unsigned it = 0, unsat = ldpc_unsatisfied(c, w.app.data());
    while (unsat != 0 && it < (unsigned)max_iter) {
        for (int r = 0; r < c.mb; r++)
            for (int i = 0; i < Z; i++)
                ldpc_row_update(w.app.data(), w.msg.data(), c.cells.data(), c.row_start[r], c.row_start[r + 1] - c.row_start[r], Z, i, a, beta);
        for (int v = 0; v < n; v++) peak = abs((int)w.app[v]) > peak ? abs((int)w.app[v]) : peak;
        it++;
        unsat = ldpc_unsatisfied(c, w.app.data());
    }
    if (bytes) {
        memset(bytes, 0, (size_t)c.k_bytes());
        for (int v = 0; v < c.k; v++) bytes[v >> 3] |= (uint8_t)((w.app[v] < 0) << (7 - (v & 7)));
    }
    if (rec) {
        unsigned flips = 0;
        for (int v = 0; v < n; v++) flips += w.L[v] != 0 && (w.app[v] < 0) != (w.L[v] < 0);
        rec[0] = it, rec[1] = unsat, rec[2] = flips;
    }
    if (status) *status = unsat == 0 ? LDPC_OK : LDPC_NOT_CONVERGED;
    return peak;
}

}  // namespace sfe
