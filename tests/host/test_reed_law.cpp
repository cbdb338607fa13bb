// The Reed-Solomon outer code's serial law (simplefe_amd/csrc/reed_law.h: reed_check, reed_encode_frame, reed_decode_frame)
// over cases read from a file, for a build with -fsanitize=address,undefined (tests/test_reed_host.py builds and runs it,
// and compares what it writes with the numpy restatement of the law).  Every buffer is a heap block of exactly the size the
// contract names, so a store or a load one byte outside is a report.
//   test_reed_law <in> <out>
// <in>: cases one after the other, each eight int32 (prim, fcr, step, n, n_par, depth, n_frames, flags: 1 encode, 2 a
// whitening sequence follows, 4 a status table follows), then the frame's Fb whitening bytes, then n_frames int32 of
// statuses, then n_frames rows of P (encode) or Fb (decode) bytes.  <out>: per case the n_frames rows of Fb (encode) or P
// (decode) bytes and, decoding, n_frames records of two uint32 and n_frames int32 statuses.  Each frame is decoded a second
// time with every output null, which must change nothing.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../simplefe_amd/csrc/reed_law.h"

using namespace sfe;

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int cases = 0;
    for (;;) {
        int32_t h[8];
        if (fread(h, sizeof(h), 1, in) != 1) break;
        ReedCode c;
        char msg[160];
        if (reed_check(h[0], h[1], h[2], h[3], h[4], h[5], &c, msg, sizeof msg) != 0) {
            printf("case %d: %s\n", cases, msg);
            return 1;
        }
        const size_t nf = (size_t)h[6], P = (size_t)c.payload_bytes(), Fb = (size_t)c.frame_bytes();
        const bool encode = h[7] & 1;
        const size_t in_row = encode ? P : Fb, out_row = encode ? Fb : P;
        uint8_t *wh = (h[7] & 2) ? (uint8_t *)malloc(Fb) : nullptr;
        int32_t *sin = (h[7] & 4) ? (int32_t *)malloc(nf * sizeof(int32_t)) : nullptr;
        uint8_t *rows = (uint8_t *)malloc(nf * in_row), *res = (uint8_t *)malloc(nf * out_row);
        uint32_t *rec = (uint32_t *)malloc(nf * 2 * sizeof(uint32_t));
        int *st = (int *)malloc(nf * sizeof(int));
        if (!rows || !res || !rec || !st || (wh && fread(wh, 1, Fb, in) != Fb) || (sin && fread(sin, sizeof(int32_t), nf, in) != nf) ||
            fread(rows, 1, nf * in_row, in) != nf * in_row)
            return 3;
        memset(res, 0xa5, nf * out_row);
        memset(rec, 0xa5, nf * 2 * sizeof(uint32_t));
        memset(st, 0xa5, nf * sizeof(int));
        for (size_t b = 0; b < nf; b++) {
            if (encode) {
                reed_encode_frame(c, wh, rows + b * in_row, res + b * out_row);
            } else {
                reed_decode_frame(c, wh, rows + b * in_row, sin && sin[b] != 0, res + b * out_row, rec + 2 * b, st + b);
                reed_decode_frame(c, wh, rows + b * in_row, sin && sin[b] != 0, nullptr, nullptr, nullptr);
            }
        }
        fwrite(res, 1, nf * out_row, out);
        if (!encode) {
            fwrite(rec, sizeof(uint32_t), nf * 2, out);
            fwrite(st, sizeof(int), nf, out);
        }
        free(wh);
        free(sin);
        free(rows);
        free(res);
        free(rec);
        free(st);
        cases++;
    }
    fclose(in);
    if (fclose(out)) return 3;
    printf("reed law ok: %d cases\n", cases);
    return 0;
}
