// reed_law.h -- the law of the Reed-Solomon outer code (sfe_dsp_reed_*, include/sfe_dsp.h), compiled by reed.hip for the
// device, by api_reed.hip for sfe_dsp_reed_plan on the host, and by tests/host/test_reed_law.cpp with a plain host compiler.
// What the two sides share is the first half: the field multiply, the limits, and the tables of a validated code (roots,
// generator, per-position locators).  The second half is the host's serial statement of encode and decode on one codeword
// and on one frame.  The law names no algorithm -- "the unique codeword within distance t, if there is one" -- so the serial
// decoder here (Berlekamp-Massey with an inverse, a root search over the n positions, Forney) and the kernel's (the
// inversion-free recurrence across lanes) give the same bytes by theorem, not by running the same steps.
// Integer arithmetic only: there is nothing here for a compiler to contract.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define REED_HD __host__ __device__
#else
#define REED_HD
#endif

namespace sfe {

constexpr int REED_MIN_N = 3, REED_MAX_N = 255, REED_MIN_PAR = 2, REED_MAX_PAR = 64, REED_MAX_DEPTH = 16;
constexpr int REED_MAX_FRAME = REED_MAX_N * REED_MAX_DEPTH;        // 4080 bytes
constexpr int REED_OK = 0, REED_UNCORRECTABLE = 1, REED_UPSTREAM = 2;

// a * b in GF(2^8) modulo the 9-bit polynomial prim: shift and xor, no table
REED_HD inline unsigned reed_mul(unsigned a, unsigned b, unsigned prim)
{
    unsigned r = 0;
#ifdef __HIP_DEVICE_COMPILE__
#pragma unroll
#endif
    for (int i = 0; i < 8; i++) {
        r ^= (0u - ((b >> i) & 1u)) & a;
        a <<= 1;
        a ^= (0u - ((a >> 8) & 1u)) & prim;
    }
    return r;
}

inline unsigned reed_pow(unsigned a, unsigned e, unsigned prim)
{
    unsigned r = 1;
    for (; e; e >>= 1, a = reed_mul(a, a, prim))
        if (e & 1u) r = reed_mul(r, a, prim);
    return r;
}
inline unsigned reed_inv(unsigned a, unsigned prim) { return reed_pow(a, 254, prim); }

// A validated code and what follows from it.  Byte j of a codeword is the coefficient of x^(n-1-j), so an error of value e
// at byte j adds e X_j^(fcr+i) to syndrome i, X_j = alpha^(step (n-1-j)): with Y = e X^fcr the syndromes are the power
// sums  S_i = sum Y X^i, the locator polynomial prod (1 - X x) has its roots at z_j = 1 / X_j, and Forney's formula reads
// Y = X Omega(z) / Lambda'(z), that is  e = Omega(z) X^(1-fcr) / Lambda'(z).
struct ReedCode {
    int prim, fcr, step, n, n_par, depth, k, t;
    uint8_t root[REED_MAX_PAR];         // alpha^(step (fcr + i))
    uint8_t gen[REED_MAX_PAR + 1];      // g(x) = prod (x - root_i): gen[l] is the coefficient of x^l, gen[n_par] = 1
    uint8_t zinv[REED_MAX_N + 1];       // z_j = 1 / X_j
    uint8_t xf[REED_MAX_N + 1];         // X_j^(1 - fcr)
    int payload_bytes() const { return depth * k; }
    int frame_bytes() const { return depth * n; }
};

// The argument checker of plan and create.  0, or -1 with a message (without the "reed: " prefix) in msg.
inline int reed_check(int prim, int fcr, int step, int n, int n_par, int depth, ReedCode *c, char *msg, size_t msg_len)
{
    if (prim < 0x100 || prim > 0x1ff) {
        snprintf(msg, msg_len, "prim = 0x%x must be a 9-bit polynomial in [0x100, 0x1ff]", (unsigned)prim);
        return -1;
    }
    int order = 0;
    for (unsigned x = 1, i = 1; i <= 255; i++) {
        x = reed_mul(x, 2, (unsigned)prim);
        if (x == 1) {
            order = (int)i;
            break;
        }
    }
    if (order != 255) {
        snprintf(msg, msg_len, "prim = 0x%x: the element 0x02 must have order 255 (it has %d; 0 = none)", (unsigned)prim, order);
        return -1;
    }
    if (n < REED_MIN_N || n > REED_MAX_N) {
        snprintf(msg, msg_len, "n = %d must be in [%d, %d]", n, REED_MIN_N, REED_MAX_N);
        return -1;
    }
    if (n_par < REED_MIN_PAR || n_par > REED_MAX_PAR || n_par >= n) {
        snprintf(msg, msg_len, "n_par = %d must be in [%d, %d] and below n = %d", n_par, REED_MIN_PAR, REED_MAX_PAR, n);
        return -1;
    }
    if (fcr < 0 || fcr > 254) {
        snprintf(msg, msg_len, "fcr = %d must be in [0, 254]", fcr);
        return -1;
    }
    if (step < 1 || step > 254 || step % 3 == 0 || step % 5 == 0 || step % 17 == 0) {
        snprintf(msg, msg_len, "step = %d must be in [1, 254] with gcd(step, 255) = 1", step);
        return -1;
    }
    if (depth < 1 || depth > REED_MAX_DEPTH) {
        snprintf(msg, msg_len, "depth = %d must be in [1, %d]", depth, REED_MAX_DEPTH);
        return -1;
    }
    const unsigned p = (unsigned)prim;
    *c = ReedCode{};
    c->prim = prim, c->fcr = fcr, c->step = step, c->n = n, c->n_par = n_par, c->depth = depth, c->k = n - n_par, c->t = n_par / 2;
    for (int i = 0; i < n_par; i++) c->root[i] = (uint8_t)reed_pow(2, (unsigned)(step * (fcr + i)) % 255u, p);
    c->gen[0] = 1;
    for (int i = 0; i < n_par; i++) {               // times (x + root_i)
        for (int l = i + 1; l >= 1; l--) c->gen[l] = (uint8_t)(c->gen[l - 1] ^ reed_mul(c->gen[l], c->root[i], p));
        c->gen[0] = (uint8_t)reed_mul(c->gen[0], c->root[i], p);
    }
    for (int j = 0; j < n; j++) {
        const unsigned e = (unsigned)(step * (n - 1 - j)) % 255u;
        c->zinv[j] = (uint8_t)reed_pow(2, (255u - e) % 255u, p);
        c->xf[j] = (uint8_t)reed_pow(2, e * ((256u - (unsigned)fcr) % 255u) % 255u, p);
    }
    return 0;
}

// ---- the serial statement, one codeword: r[0 .. n) contiguous

// the last n_par bytes of r become x^n_par m(x) mod g(x), m the first k bytes
inline void reed_encode_word(const ReedCode &c, uint8_t *r)
{
    const unsigned p = (unsigned)c.prim;
    uint8_t rem[REED_MAX_PAR] = {};                 // rem[l]: the coefficient of x^l
    for (int j = 0; j < c.k; j++) {
        const unsigned fb = r[j] ^ rem[c.n_par - 1];
        for (int l = c.n_par - 1; l >= 1; l--) rem[l] = (uint8_t)(rem[l - 1] ^ reed_mul(fb, c.gen[l], p));
        rem[0] = (uint8_t)reed_mul(fb, c.gen[0], p);
    }
    for (int l = 0; l < c.n_par; l++) r[c.k + (c.n_par - 1 - l)] = rem[l];
}

inline unsigned reed_eval(const uint8_t *poly, int deg, unsigned z, unsigned p)      // poly[l]: the coefficient of x^l
{
    unsigned v = 0;
    for (int l = deg; l >= 0; l--) v = reed_mul(v, z, p) ^ poly[l];
    return v;
}

// The codeword of C within distance t of r, if there is one: r becomes it and its distance is returned; -1 and r
// untouched otherwise.
inline int reed_decode_word(const ReedCode &c, uint8_t *r)
{
    const unsigned p = (unsigned)c.prim;
    const int np = c.n_par;
    uint8_t S[REED_MAX_PAR];
    bool clean = true;
    for (int i = 0; i < np; i++) {
        unsigned s = 0;
        for (int j = 0; j < c.n; j++) s = reed_mul(s, c.root[i], p) ^ r[j];
        S[i] = (uint8_t)s;
        clean = clean && s == 0;
    }
    if (clean) return 0;
    // the shortest recurrence of the syndromes
    uint8_t C[REED_MAX_PAR + 2] = {1}, B[REED_MAX_PAR + 2] = {1}, T[REED_MAX_PAR + 2];
    int L = 0, m = 1;
    unsigned b = 1;
    for (int k = 0; k < np; k++) {
        unsigned d = S[k];
        for (int i = 1; i <= L; i++) d ^= reed_mul(C[i], S[k - i], p);
        if (d == 0) {
            m++;
            continue;
        }
        const unsigned coef = reed_mul(d, reed_inv(b, p), p);
        memcpy(T, C, sizeof(T));
        for (int i = 0; i + m <= np; i++) C[i + m] ^= (uint8_t)reed_mul(coef, B[i], p);
        if (2 * L <= k) {
            L = k + 1 - L;
            memcpy(B, T, sizeof(B));
            b = d;
            m = 1;
        } else {
            m++;
        }
    }
    if (L > c.t) return -1;
    int deg = np;
    while (deg > 0 && C[deg] == 0) deg--;
    if (deg != L) return -1;
    // its roots among the n positions of the code: a root at a padded position of a shortened code is no position at all
    int pos[REED_MAX_PAR], found = 0;
    for (int j = 0; j < c.n; j++)
        if (reed_eval(C, L, c.zinv[j], p) == 0) {
            if (found == L) return -1;
            pos[found++] = j;
        }
    if (found != L) return -1;
    uint8_t Om[REED_MAX_PAR] = {}, D[REED_MAX_PAR] = {};        // Omega = S Lambda mod x^L; D: Lambda' in w = x^2
    for (int i = 0; i < L; i++)
        for (int l = 0; l <= i; l++) Om[i] ^= (uint8_t)reed_mul(C[l], S[i - l], p);
    for (int l = 1; l <= L; l += 2) D[l / 2] = C[l];
    for (int q = 0; q < L; q++) {
        const unsigned z = c.zinv[pos[q]];
        const unsigned den = reed_eval(D, (L - 1) / 2, reed_mul(z, z, p), p);
        const unsigned e = reed_mul(reed_mul(reed_eval(Om, L - 1, z, p), c.xf[pos[q]], p), reed_inv(den, p), p);
        r[pos[q]] ^= (uint8_t)e;
    }
    return L;
}

// ---- one frame.  whiten: frame_bytes() bytes or null.

inline void reed_encode_frame(const ReedCode &c, const uint8_t *whiten, const uint8_t *payload, uint8_t *frame)
{
    uint8_t w[REED_MAX_N];
    for (int i = 0; i < c.depth; i++) {
        for (int j = 0; j < c.k; j++) w[j] = payload[j * c.depth + i];
        reed_encode_word(c, w);
        for (int j = 0; j < c.n; j++) frame[j * c.depth + i] = (uint8_t)(w[j] ^ (whiten ? whiten[j * c.depth + i] : 0));
    }
}

// out (payload_bytes()), rec (two words) and status may each be null
inline void reed_decode_frame(const ReedCode &c, const uint8_t *whiten, const uint8_t *frame, bool upstream, uint8_t *out, uint32_t *rec, int *status)
{
    if (upstream) {
        if (out) memset(out, 0, (size_t)c.payload_bytes());
        if (rec) rec[0] = 0, rec[1] = (1u << c.depth) - 1u;
        if (status) *status = REED_UPSTREAM;
        return;
    }
    uint8_t w[REED_MAX_N];
    uint32_t sum = 0, bad = 0;
    for (int i = 0; i < c.depth; i++) {
        for (int j = 0; j < c.n; j++) w[j] = (uint8_t)(frame[j * c.depth + i] ^ (whiten ? whiten[j * c.depth + i] : 0));
        const int d = reed_decode_word(c, w);
        if (d < 0) bad |= 1u << i;
        else sum += (uint32_t)d;
        if (out)
            for (int j = 0; j < c.k; j++) out[j * c.depth + i] = w[j];
    }
    if (rec) rec[0] = sum, rec[1] = bad;
    if (status) *status = bad ? REED_UNCORRECTABLE : REED_OK;
}

}  // namespace sfe
