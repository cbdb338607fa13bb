// The quasi-cyclic LDPC code's serial law (simplefe_amd/csrc/ldpc_law.h: ldpc_check, ldpc_build_encoder, ldpc_encode_word,
// ldpc_decode_word) over cases read from a file, for a build with -fsanitize=address,undefined (tests/test_ldpc_host.py
// builds and runs it, and compares what it writes with the numpy restatement of the law).  Every buffer is a heap block of
// exactly the size the contract names, so a store or a load one byte outside is a report.
//   test_ldpc_law <in> <out>
// <in>: cases one after the other, each eight int32 (mb, nb, Z, a, beta, max_iter, n_words, flags: 1 encode, 4 a status
// table follows), a float32 scale, the mb nb int16 of the base matrix, then n_words int32 of statuses, then n_words rows of
// ceil(k / 8) bytes (encode) or n float32 (decode).  <out>: per case the n_words rows of ceil(n / 8) (encode) or ceil(k / 8)
// (decode) bytes and, decoding, n_words records of three uint32 and n_words int32 statuses.  Each word is decoded a second
// time with every output null, which must change nothing.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../simplefe_amd/csrc/ldpc_law.h"

using namespace sfe;

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int cases = 0;
    for (;;) {
        int32_t h[8];
        float scale;
        if (fread(h, sizeof(h), 1, in) != 1) break;
        if (fread(&scale, sizeof(scale), 1, in) != 1) return 3;
        const size_t cells = (size_t)h[0] * (size_t)h[1];
        int16_t *shift = (int16_t *)malloc(cells * sizeof(int16_t));
        if (!shift || fread(shift, sizeof(int16_t), cells, in) != cells) return 3;
        LdpcCode c;
        char msg[160];
        if (ldpc_check(h[0], h[1], h[2], shift, &c, msg, sizeof msg) != 0 || ldpc_check_params(scale, h[3], h[4], h[5], msg, sizeof msg) != 0) {
            printf("case %d: %s\n", cases, msg);
            return 1;
        }
        ldpc_build_encoder(&c);
        const size_t nw = (size_t)h[6], kb = (size_t)c.k_bytes(), nb = (size_t)c.n_bytes(), n = (size_t)c.n;
        const bool encode = h[7] & 1;
        if (encode && !c.encodable) {
            printf("case %d: not encodable\n", cases);
            return 1;
        }
        const size_t in_row = encode ? kb : n * sizeof(float), out_row = encode ? nb : kb;
        int32_t *sin = (h[7] & 4) ? (int32_t *)malloc(nw * sizeof(int32_t)) : nullptr;
        uint8_t *rows = (uint8_t *)malloc(nw * in_row), *res = (uint8_t *)malloc(nw * out_row);
        uint32_t *rec = (uint32_t *)malloc(nw * 3 * sizeof(uint32_t));
        int *st = (int *)malloc(nw * sizeof(int));
        if (!rows || !res || !rec || !st || (sin && fread(sin, sizeof(int32_t), nw, in) != nw) || fread(rows, 1, nw * in_row, in) != nw * in_row) return 3;
        memset(res, 0xa5, nw * out_row);
        memset(rec, 0xa5, nw * 3 * sizeof(uint32_t));
        memset(st, 0xa5, nw * sizeof(int));
        LdpcWork w;
        for (size_t b = 0; b < nw; b++) {
            if (encode) {
                ldpc_encode_word(c, rows + b * in_row, res + b * out_row);
            } else if (sin && sin[b] != 0) {
                ldpc_fail_word(c, LDPC_UPSTREAM, res + b * out_row, rec + 3 * b, st + b);
            } else {
                const float *row = reinterpret_cast<const float *>(rows + b * in_row);
                ldpc_decode_word(c, w, row, 1, scale, h[3], h[4], h[5], res + b * out_row, rec + 3 * b, st + b);
                ldpc_decode_word(c, w, row, 1, scale, h[3], h[4], h[5], nullptr, nullptr, nullptr);
            }
        }
        fwrite(res, 1, nw * out_row, out);
        if (!encode) {
            fwrite(rec, sizeof(uint32_t), nw * 3, out);
            fwrite(st, sizeof(int), nw, out);
        }
        free(shift);
        free(sin);
        free(rows);
        free(res);
        free(rec);
        free(st);
        cases++;
    }
    fclose(in);
    if (fclose(out)) return 3;
    printf("ldpc law ok: %d cases\n", cases);
    return 0;
}
