// crc_law.h -- the law of the frame check (sfe_dsp_crc_*, include/sfe_dsp.h): a CRC of width 8, 16, 24 or 32 behind a payload
// and an additive, frame-synchronous scrambler over the whole frame.  Compiled by crc.hip for the device, by api_crc.hip for
// sfe_dsp_crc_plan on the host, and by tests/host/test_crc_law.cpp with a plain host compiler.
// The first half is the law as the header states it, bit by bit (crc_serial, crc_pn_bytes): nothing else defines the bytes.
// The second half is arithmetic both sides build their fast forms from.  A register of width w is kept LEFT-ALIGNED in 32
// bits, R = r << (32 - w): the shift register of the law is then, for every width, multiplication by x modulo
// G'(x) = x^32 + polyL(x), polyL = poly << (32 - w), in the ring of polynomials over GF(2) of degree below 32 -- G' is G times
// x^(32 - w), not irreducible, and nothing below needs it to be.  In that ring the register after a message M of n bytes from
// a zero start is M(x) x^32 mod G', so the contributions of the pieces of a message add, each shifted by x^(8 k) for the k
// bytes behind it, and a non-zero init adds initL x^(8 n): what the kernels fold across lanes, and what the host plan's
// byte table (crc_table) is one column of.
// Integer arithmetic only: there is nothing here for a compiler to contract.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define CRC_HD __host__ __device__
#else
#define CRC_HD
#endif

namespace sfe {

constexpr int CRC_MAX_PAYLOAD = 1 << 20, CRC_MIN_PN = 2, CRC_MAX_PN = 32;
constexpr int CRC_OK = 0, CRC_MISMATCH = 1, CRC_UPSTREAM = 2;

struct CrcLaw {
    int width;                  // 0 (no CRC), 8, 16, 24, 32
    uint32_t poly, init, xorout;
    int reflect;
    int pn_m;                   // 0 (no scrambler), 2 .. 32
    uint32_t pn_taps, pn_seed;
    int payload;                // P
    CRC_HD int tail_bytes() const { return width / 8; }
    CRC_HD int frame_bytes() const { return payload + width / 8; }
    CRC_HD uint32_t mask() const { return width == 32 ? 0xffffffffu : (1u << width) - 1u; }
    CRC_HD uint32_t polyL() const { return width ? poly << (32 - width) : 0u; }
    CRC_HD uint32_t initL() const { return width ? init << (32 - width) : 0u; }
};

// The argument checker of plan and create.  0, or -1 with a message (without the "crc: " prefix) in msg.
inline int crc_check_args(int width, uint32_t poly, uint32_t init, int reflect, uint32_t xorout, int pn_m, uint32_t pn_taps, uint32_t pn_seed,
                          int payload, CrcLaw *c, char *msg, size_t msg_len)
{
    if (width != 0 && width != 8 && width != 16 && width != 24 && width != 32) {
        snprintf(msg, msg_len, "width = %d must be 0 (no CRC), 8, 16, 24 or 32", width);
        return -1;
    }
    if (width == 0 && pn_m == 0) {
        snprintf(msg, msg_len, "width = 0 and pn_m = 0: a handle with neither a CRC nor a scrambler");
        return -1;
    }
    const uint32_t mask = width == 32 ? 0xffffffffu : (1u << width) - 1u;
    if (width && (!(poly & 1u) || poly > mask)) {
        snprintf(msg, msg_len, "poly = 0x%x must have bit 0 set and lie below 2^%d (the top term is implicit)", poly, width);
        return -1;
    }
    if (width && (init > mask || xorout > mask)) {
        snprintf(msg, msg_len, "init = 0x%x and xorout = 0x%x must lie below 2^%d", init, xorout, width);
        return -1;
    }
    if (reflect != 0 && reflect != 1) {
        snprintf(msg, msg_len, "reflect = %d is neither 0 nor 1", reflect);
        return -1;
    }
    if (pn_m != 0 && (pn_m < CRC_MIN_PN || pn_m > CRC_MAX_PN)) {
        snprintf(msg, msg_len, "pn_m = %d must be 0 (no scrambler) or in [%d, %d]", pn_m, CRC_MIN_PN, CRC_MAX_PN);
        return -1;
    }
    if (pn_m) {
        const uint32_t pm = pn_m == 32 ? 0xffffffffu : (1u << pn_m) - 1u;
        if (!(pn_taps & 1u) || pn_taps > pm) {
            snprintf(msg, msg_len, "pn_taps = 0x%x must have bit 0 set and lie below 2^%d", pn_taps, pn_m);
            return -1;
        }
        if (pn_seed == 0 || pn_seed > pm) {
            snprintf(msg, msg_len, "pn_seed = 0x%x must lie in [1, 2^%d)", pn_seed, pn_m);
            return -1;
        }
    }
    if (payload < 1 || payload > CRC_MAX_PAYLOAD) {
        snprintf(msg, msg_len, "payload_bytes = %d must be in [1, 2^20]", payload);
        return -1;
    }
    *c = CrcLaw{width, width ? poly : 0u, width ? init : 0u, width ? xorout : 0u, width ? reflect : 0, pn_m, pn_m ? pn_taps : 0u,
                pn_m ? pn_seed : 0u, payload};
    return 0;
}

// ---- the law, bit by bit

CRC_HD inline uint32_t crc_rev32(uint32_t v)
{
#if defined(__clang__)
    return __builtin_bitreverse32(v);
#else
    v = (v >> 16) | (v << 16);
    v = ((v & 0xff00ff00u) >> 8) | ((v & 0x00ff00ffu) << 8);
    v = ((v & 0xf0f0f0f0u) >> 4) | ((v & 0x0f0f0f0fu) << 4);
    v = ((v & 0xccccccccu) >> 2) | ((v & 0x33333333u) << 2);
    return ((v & 0xaaaaaaaau) >> 1) | ((v & 0x55555555u) << 1);
#endif
}
CRC_HD inline uint32_t crc_rev8(uint32_t b) { return crc_rev32(b) >> 24; }

// the CRC of n bytes: the header's sentences in their order, the register right-aligned as they state it
inline uint32_t crc_serial(const CrcLaw &c, const uint8_t *p, size_t n)
{
    const int w = c.width;
    if (!w) return 0;
    const uint32_t mask = c.mask(), top = 1u << (w - 1);
    uint32_t r = c.init;
    for (size_t j = 0; j < n; j++) {
        const uint32_t b = c.reflect ? crc_rev8(p[j]) : p[j];
        r ^= b << (w - 8);
        for (int i = 0; i < 8; i++) r = (r & top) ? ((r << 1) ^ c.poly) & mask : (r << 1) & mask;
    }
    if (c.reflect) r = crc_rev32(r) >> (32 - w);
    return r ^ c.xorout;
}

// n bytes of the scrambler's sequence: a[i] = bit i of seed for i < m, a[n + m] = the xor over the set bits i of taps of
// a[n + i]; a[8 j] is bit 7 of byte j.  s holds a[n .. n + m), a[n + i] in bit i.
inline void crc_pn_bytes(int m, uint32_t taps, uint32_t seed, size_t n, uint8_t *out)
{
    uint32_t s = seed;
    for (size_t j = 0; j < n; j++) {
        unsigned byte = 0;
        for (int k = 7; k >= 0; k--) {
            byte |= (s & 1u) << k;
            const uint32_t fresh = (uint32_t)__builtin_parity(s & taps);
            s = (s >> 1) | (fresh << (m - 1));
        }
        out[j] = (uint8_t)byte;
    }
}

// ---- the ring: registers left-aligned

CRC_HD inline uint32_t crc_mulx(uint32_t R, uint32_t polyL) { return (R << 1) ^ ((0u - (R >> 31)) & polyL); }     // R x mod G'

// the register after byte b (as the law feeds it: bit-reversed already where the model reflects)
CRC_HD inline uint32_t crc_feed(uint32_t R, uint32_t b, uint32_t polyL)
{
    R ^= b << 24;
#ifdef __HIP_DEVICE_COMPILE__
#pragma unroll
#endif
    for (int i = 0; i < 8; i++) R = crc_mulx(R, polyL);
    return R;
}

// a b mod G': Horner over b's bits
CRC_HD inline uint32_t crc_mulmod(uint32_t a, uint32_t b, uint32_t polyL)
{
    uint32_t r = 0;
#ifdef __HIP_DEVICE_COMPILE__
#pragma unroll
#endif
    for (int i = 31; i >= 0; i--) r = crc_mulx(r, polyL) ^ ((0u - ((b >> i) & 1u)) & a);
    return r;
}

// x^k mod G'
inline uint32_t crc_xpow(uint64_t k, uint32_t polyL)
{
    uint32_t r = 1u, s = 2u;
    for (; k; k >>= 1, s = crc_mulmod(s, s, polyL))
        if (k & 1u) r = crc_mulmod(r, s, polyL);
    return r;
}

// What a kernel that deals a frame's dwords round robin over T lanes needs (crc.hip): the 32 columns x^(b + 32 T) of the
// matrix that carries a lane's register over one round, then the T weights x^(32 (T - l)) of the lanes' registers in the frame's.
inline void crc_class_constants(uint32_t polyL, int T, uint32_t *tab)
{
    uint32_t v = crc_xpow(32ull * (uint64_t)T, polyL);
    for (int b = 0; b < 32; b++, v = crc_mulx(v, polyL)) tab[b] = v;
    const uint32_t x32 = crc_xpow(32, polyL);
    v = x32;                                                    // lane T - 1 first: x^32
    for (int l = T - 1; l >= 0; l--, v = crc_mulmod(v, x32, polyL)) tab[32 + l] = v;
}

// the CRC a finished register stands for
CRC_HD inline uint32_t crc_finish(uint32_t R, const CrcLaw &c)
{
    if (!c.width) return 0u;
    return (c.reflect ? crc_rev32(R) : R >> (32 - c.width)) ^ c.xorout;
}

// byte k of the w / 8 bytes behind the payload: most significant first, or least significant first where the model reflects
CRC_HD inline uint32_t crc_tail_byte(uint32_t crc, int k, const CrcLaw &c) { return (crc >> (c.reflect ? 8 * k : c.width - 8 - 8 * k)) & 0xffu; }
// and where byte k goes in the CRC read back
CRC_HD inline uint32_t crc_tail_place(uint32_t byte, int k, const CrcLaw &c) { return byte << (c.reflect ? 8 * k : c.width - 8 - 8 * k); }

// ---- the host's fast form: a byte at a time through the 256 registers a byte leaves behind
struct CrcTable {
    uint32_t t[256];
    uint8_t rev[256];           // the byte as the law feeds it
};
inline void crc_table(const CrcLaw &c, CrcTable *T)
{
    for (uint32_t b = 0; b < 256; b++) {
        T->t[b] = crc_feed(0u, b, c.polyL());
        T->rev[b] = (uint8_t)(c.reflect ? crc_rev8(b) : b);
    }
}
// the register after n more bytes
inline uint32_t crc_run(const CrcTable &T, uint32_t R, const uint8_t *p, size_t n)
{
    for (size_t j = 0; j < n; j++) R = (R << 8) ^ T.t[(R >> 24) ^ T.rev[p[j]]];
    return R;
}

// ---- one frame on the host.  pn: frame_bytes() bytes of the sequence, or null without a scrambler.
// transmit: payload || crc bytes, the whole xor pn
inline void crc_append_frame(const CrcLaw &c, const CrcTable &T, const uint8_t *pn, const uint8_t *in, uint8_t *out)
{
    const int P = c.payload, nt = c.tail_bytes();
    const uint32_t crc = crc_finish(crc_run(T, c.initL(), in, (size_t)P), c);
    if (!out) return;
    for (int q = 0; q < P; q++) out[q] = (uint8_t)(in[q] ^ (pn ? pn[q] : 0));
    for (int k = 0; k < nt; k++) out[P + k] = (uint8_t)(crc_tail_byte(crc, k, c) ^ (pn ? pn[P + k] : 0));
}

// receive: r = in xor pn, the CRC over r[0 .. P) against the one in r[P .. Fb).  Each output may be null.
inline void crc_check_frame(const CrcLaw &c, const CrcTable &T, const uint8_t *pn, const uint8_t *in, bool upstream, uint8_t *out, uint32_t *rec,
                            int *status)
{
    const int P = c.payload, nt = c.tail_bytes();
    if (upstream) {
        if (out) memset(out, 0, (size_t)P);
        if (rec) rec[0] = rec[1] = 0u;
        if (status) *status = CRC_UPSTREAM;
        return;
    }
    uint32_t R = c.initL(), got = 0u;
    for (int q = 0; q < P; q++) {
        const uint8_t b = (uint8_t)(in[q] ^ (pn ? pn[q] : 0));
        R = crc_run(T, R, &b, 1);
        if (out) out[q] = b;
    }
    for (int k = 0; k < nt; k++) got |= crc_tail_place((uint32_t)(in[P + k] ^ (pn ? pn[P + k] : 0)), k, c);
    const uint32_t crc = crc_finish(R, c);
    if (rec) rec[0] = crc, rec[1] = got;
    if (status) *status = crc == got ? CRC_OK : CRC_MISMATCH;
}

}  // namespace sfe
