// The occupancy detector's host plan (simplefe_amd/csrc/occ_law.h: occ_plan_row) over cases read from a file, for a build with
// -fsanitize=address,undefined (tests/test_occ_host.py builds and runs it, and compares what it writes with the numpy
// restatement of the law).  Every buffer is a heap block of exactly the size the contract names, so a store or a load
// one element outside is a report.
//   test_occ_law <in> <out>
// <in>: cases one after the other, each nine 32-bit words (N, R, rank, gap, min_width, E, shift as int32, factor and min_level
// as float32) and R rows of N float32.  <out>: per case R info records, R*E emission records, R*N mask bytes.  Each case runs
// a second time without the mask and with every output null, which must change nothing.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../simplefe_amd/csrc/occ_law.h"

using namespace sfe;

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int cases = 0;
    for (;;) {
        int32_t h[7];
        float f[2];
        if (fread(h, sizeof(h), 1, in) != 1) break;
        if (fread(f, sizeof(f), 1, in) != 1) return 3;
        const OccParams p{h[0], h[2], h[3], h[4], h[5], h[6], f[0], f[1]};
        const size_t N = (size_t)h[0], R = (size_t)h[1], E = (size_t)h[5];
        float *rows = (float *)malloc(R * N * sizeof(float));
        sfe_occ_info *info = (sfe_occ_info *)malloc(R * sizeof(sfe_occ_info)), *info2 = (sfe_occ_info *)malloc(R * sizeof(sfe_occ_info));
        sfe_occ_rec *rec = (sfe_occ_rec *)malloc(R * E * sizeof(sfe_occ_rec)), *rec2 = (sfe_occ_rec *)malloc(R * E * sizeof(sfe_occ_rec));
        uint8_t *mask = (uint8_t *)malloc(R * N);
        if (!rows || !info || !info2 || !rec || !rec2 || !mask || fread(rows, sizeof(float), R * N, in) != R * N) return 3;
        memset(info, 0xa5, R * sizeof(sfe_occ_info));
        memset(rec, 0xa5, R * E * sizeof(sfe_occ_rec));
        memset(mask, 0xa5, R * N);
        memset(info2, 0x5a, R * sizeof(sfe_occ_info));
        memset(rec2, 0x5a, R * E * sizeof(sfe_occ_rec));
        for (size_t i = 0; i < R; i++) {
            occ_plan_row(p, rows + i * N, info + i, rec + i * E, mask + i * N);
            occ_plan_row(p, rows + i * N, info2 + i, rec2 + i * E, nullptr);
            occ_plan_row(p, rows + i * N, nullptr, nullptr, nullptr);
        }
        if (memcmp(info, info2, R * sizeof(sfe_occ_info)) || memcmp(rec, rec2, R * E * sizeof(sfe_occ_rec))) {
            printf("case %d: info or records differ without the mask\n", cases);
            return 1;
        }
        fwrite(info, sizeof(sfe_occ_info), R, out);
        fwrite(rec, sizeof(sfe_occ_rec), R * E, out);
        fwrite(mask, 1, R * N, out);
        free(rows);
        free(info);
        free(info2);
        free(rec);
        free(rec2);
        free(mask);
        cases++;
    }
    fclose(in);
    if (fclose(out)) return 3;
    printf("occ law ok: %d cases\n", cases);
    return 0;
}
