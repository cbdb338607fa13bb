// The frame check's law (simplefe_amd/csrc/crc_law.h) against itself, for a build with -fsanitize=address,undefined
// (tests/test_crc_host.py builds and runs it): the serial statement (crc_serial), the host plan's byte table (crc_run) and
// the fold over lanes that the kernels run -- restated here on the host with the constants the handle makes at create
// (crc_class_constants, the init term) -- must give the same CRC, over the catalogue's models and over seeded shapes; then
// whole frames through crc_append_frame and crc_check_frame, from heap blocks of exactly the contract's sizes, so a store or
// a load one byte outside is a report.
//   test_crc_law          prints "crc law ok: <n> checks"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../simplefe_amd/csrc/crc_law.h"

using namespace sfe;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 16);
}

// What crc.hip does with T lanes, a lane after the other: pad zero dwords in front, rounds of T dwords, lane l's register
// carried by the columns and weighted at the end, the bytes behind the last dword fed one by one, the init term on top.
static uint32_t fold(const CrcLaw &c, int T, const uint8_t *p, size_t n)
{
    const uint32_t polyL = c.polyL();
    std::vector<uint32_t> tab(32 + (size_t)T);
    crc_class_constants(polyL, T, tab.data());
    const size_t nd = n / 4, rounds = (nd + T - 1) / T, pad = rounds * T - nd;
    uint32_t R = 0;
    for (int l = 0; l < T; l++) {
        uint32_t A = 0;
        for (size_t i = 0; i < rounds; i++) {
            const size_t v = i * T + l;
            uint32_t D = 0;
            if (v >= pad) {
                const uint8_t *q = p + 4 * (v - pad);
                const uint32_t raw = (uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16 | (uint32_t)q[3] << 24;
                D = c.reflect ? crc_rev32(raw) : (raw >> 24) | ((raw >> 8) & 0xff00u) | ((raw << 8) & 0xff0000u) | (raw << 24);
            }
            uint32_t r = 0;
            for (int b = 0; b < 32; b++) r ^= (0u - ((A >> b) & 1u)) & tab[b];
            A = r ^ D;
        }
        R ^= crc_mulmod(A, tab[32 + l], polyL);
    }
    for (size_t q = 4 * nd; q < n; q++) R = crc_feed(R, c.reflect ? crc_rev8(p[q]) : p[q], polyL);
    const uint32_t init_term = crc_mulmod(c.initL(), crc_xpow(8ull * n, polyL), polyL);
    return crc_finish(R ^ init_term, c);
}

static const uint32_t MODELS[][5] = {
    {32, 0x04C11DB7u, 0xFFFFFFFFu, 1, 0xFFFFFFFFu}, {32, 0x1EDC6F41u, 0xFFFFFFFFu, 1, 0xFFFFFFFFu}, {32, 0x04C11DB7u, 0xFFFFFFFFu, 0, 0},
    {32, 0x04C11DB7u, 0xFFFFFFFFu, 0, 0xFFFFFFFFu}, {24, 0x864CFBu, 0xB704CEu, 0, 0}, {24, 0x864CFBu, 0, 0, 0}, {16, 0x1021u, 0, 0, 0},
    {16, 0x1021u, 0xFFFFu, 0, 0}, {16, 0x1021u, 0, 1, 0}, {16, 0x8005u, 0, 1, 0}, {16, 0x1021u, 0xFFFFu, 1, 0xFFFFu}, {8, 0x07u, 0, 0, 0},
    {8, 0x31u, 0, 1, 0}};
static const uint32_t CHECKS[] = {0xCBF43926u, 0xE3069283u, 0x0376E6E7u, 0xFC891918u, 0x21CF02u, 0xCDE703u, 0x31C3u,
                                  0x29B1u,     0x2189u,     0xBB3Du,     0x906Eu,     0xF4u,     0xA1u};

static int checks = 0;

static int one(const CrcLaw &c, size_t n)
{
    uint8_t *p = (uint8_t *)malloc(n);
    if (!p) return 3;
    for (size_t i = 0; i < n; i++) p[i] = (uint8_t)rnd();
    CrcTable T;
    crc_table(c, &T);
    const uint32_t want = crc_serial(c, p, n), fast = crc_finish(crc_run(T, c.initL(), p, n), c);
    const uint32_t f64 = fold(c, 64, p, n), f1024 = fold(c, 1024, p, n);
    free(p);
    checks++;
    if (fast != want || f64 != want || f1024 != want) {
        printf("w %d poly %x init %x reflect %d xorout %x, %zu bytes: serial %x table %x fold64 %x fold1024 %x\n", c.width, c.poly, c.init,
               c.reflect, c.xorout, n, want, fast, f64, f1024);
        return 1;
    }
    return 0;
}

static int frames(const CrcLaw &c)
{
    const size_t P = (size_t)c.payload, Fb = (size_t)c.frame_bytes();
    uint8_t *pay = (uint8_t *)malloc(P), *frm = (uint8_t *)malloc(Fb), *back = (uint8_t *)malloc(P), *pn = c.pn_m ? (uint8_t *)malloc(Fb) : nullptr;
    if (!pay || !frm || !back) return 3;
    for (size_t i = 0; i < P; i++) pay[i] = (uint8_t)rnd();
    if (pn) crc_pn_bytes(c.pn_m, c.pn_taps, c.pn_seed, Fb, pn);
    CrcTable T;
    crc_table(c, &T);
    crc_append_frame(c, T, pn, pay, frm);
    uint32_t rec[2] = {1, 2};
    int st = -1, bad = 0;
    crc_check_frame(c, T, pn, frm, false, back, rec, &st);
    crc_check_frame(c, T, pn, frm, false, nullptr, nullptr, nullptr);
    bad |= st != CRC_OK || rec[0] != rec[1] || rec[0] != crc_serial(c, pay, P) || memcmp(back, pay, P) != 0;
    frm[rnd() % Fb] ^= (uint8_t)(1u << (rnd() % 8));
    crc_check_frame(c, T, pn, frm, false, back, rec, &st);
    bad |= c.width ? st != CRC_MISMATCH : st != CRC_OK;
    crc_check_frame(c, T, pn, frm, true, back, rec, &st);
    bad |= st != CRC_UPSTREAM || rec[0] || rec[1];
    for (size_t i = 0; i < P; i++) bad |= back[i] != 0;
    free(pay);
    free(frm);
    free(back);
    free(pn);
    checks++;
    if (bad) printf("frames: w %d poly %x reflect %d pn_m %d P %zu\n", c.width, c.poly, c.reflect, c.pn_m, P);
    return bad;
}

int main()
{
    char msg[200];
    const size_t lengths[] = {1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 255, 256, 257, 259, 1020, 1023, 1024, 1025, 4095, 4096, 4097, 4099, 8191, 8192, 8193, 65541};
    for (size_t m = 0; m < sizeof(MODELS) / sizeof(MODELS[0]); m++) {
        CrcLaw c;
        if (crc_check_args((int)MODELS[m][0], MODELS[m][1], MODELS[m][2], (int)MODELS[m][3], MODELS[m][4], 0, 0, 0, 9, &c, msg, sizeof msg) != 0) {
            printf("model %zu: %s\n", m, msg);
            return 1;
        }
        const uint8_t *nine = (const uint8_t *)"123456789";
        if (crc_serial(c, nine, 9) != CHECKS[m] || fold(c, 64, nine, 9) != CHECKS[m]) {
            printf("model %zu: check value %x, not %x\n", m, crc_serial(c, nine, 9), CHECKS[m]);
            return 1;
        }
        checks++;
        for (size_t n : lengths)
            if (one(c, n)) return 1;
        for (int pn_m : {0, 8, 32}) {
            for (int P : {1, 3, 24, 1021}) {
                CrcLaw f;
                if (crc_check_args(c.width, c.poly, c.init, c.reflect, c.xorout, pn_m, pn_m == 32 ? 0x00400007u : 0xA9u, 0xFFu, P, &f, msg, sizeof msg) != 0) return 1;
                if (frames(f)) return 1;
            }
        }
    }
    // seeded shapes: any odd polynomial, any init and xorout, either reflection
    for (int k = 0; k < 300; k++) {
        const int w = 8 * (1 + (int)(rnd() % 4));
        const uint32_t mask = w == 32 ? 0xffffffffu : (1u << w) - 1u;
        CrcLaw c;
        if (crc_check_args(w, (rnd() & mask) | 1u, rnd() & mask, (int)(rnd() & 1u), rnd() & mask, 0, 0, 0, 1, &c, msg, sizeof msg) != 0) return 1;
        if (one(c, 1 + rnd() % 9000)) return 1;
    }
    CrcLaw s;                                   // a scrambler alone
    if (crc_check_args(0, 0, 0, 0, 0, 7, 0x09u, 0x7Fu, 37, &s, msg, sizeof msg) != 0 || frames(s)) return 1;
    printf("crc law ok: %d checks\n", checks);
    return 0;
}
