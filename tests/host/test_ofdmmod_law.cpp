// The OFDM modulator's law (simplefe_amd/csrc/ofdmmod_law.h: the bins, the transform, the frame and the wire format) over
// cases read from a file, for a build with -fsanitize=address,undefined (tests/test_ofdmmod_host.py builds and runs it, and
// compares what it writes with sfe_dsp_ofdmmod_plan's bytes).  Every buffer is a heap block of exactly the size the contract
// names, so a store or a load one element outside is a report.
//   test_ofdmmod_law <in> <out>
// <in>: cases one after the other, each eight 32-bit words (log2 N, cp, T, Ns, order, symbols, tx10, rows as int32), amp as
// float32, then src [N] int32, ta [N] cf32, pa [N] cf32, sign [Ns] float32 and `rows` input rows of exactly what a burst reads
// (bytes, or cf32 symbols).  <out>: per row its frame, F cf32 or (F / 2) * 5 bytes.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../simplefe_amd/csrc/ofdmmod_law.h"

using namespace sfe;

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int cases = 0;
    for (;;) {
        int32_t h[8];
        float amp;
        if (fread(h, sizeof(h), 1, in) != 1) break;
        if (fread(&amp, sizeof(amp), 1, in) != 1) return 3;
        const int logn = h[0], cp = h[1], T = h[2], Ns = h[3], order = h[4], symbols = h[5], tx10 = h[6], rows = h[7];
        const size_t N = (size_t)1 << logn, F = (size_t)(T + Ns) * (N + (size_t)cp);
        omc *tw = (omc *)malloc(N * sizeof(omc)), *ta = (omc *)malloc(N * sizeof(omc)), *pa = (omc *)malloc(N * sizeof(omc));
        omc *v = (omc *)malloc(N * sizeof(omc)), *tmp = (omc *)malloc(N * sizeof(omc)), *y = (omc *)malloc(F * sizeof(omc));
        float *sign = (float *)malloc((size_t)Ns * sizeof(float));
        int *src = (int *)malloc(N * sizeof(int));
        uint8_t *wire = (uint8_t *)malloc(F / 2 * 5 + 1);
        if (!tw || !ta || !pa || !v || !tmp || !y || !sign || !src || !wire) return 3;
        if (fread(src, sizeof(int), N, in) != N || fread(ta, sizeof(omc), N, in) != N || fread(pa, sizeof(omc), N, in) != N ||
            fread(sign, sizeof(float), (size_t)Ns, in) != (size_t)Ns)
            return 3;
        int Nd = 0;
        for (size_t k = 0; k < N; k++) Nd += src[k] >= 0;
        om_twiddles((int)N, tw);
        const float a = order == 2 ? amp : (float)((double)amp / sqrt(2.0));
        const OmodLaw law{tw, ta, pa, sign, src, logn, cp, T, Ns, Nd, order, symbols, amp, a};
        const size_t n_in = symbols ? (size_t)Ns * Nd * sizeof(omc) : ((size_t)Ns * Nd * (order == 4 ? 2 : 1) + 7) / 8;
        for (int r = 0; r < rows; r++) {
            void *row = malloc(n_in);
            if (!row || fread(row, 1, n_in, in) != n_in) return 3;
            om_frame_host(law, row, v, tmp, y);
            if (tx10) {
                om_tx10_host(y, F, wire);
                fwrite(wire, 1, F / 2 * 5, out);
            } else {
                fwrite(y, sizeof(omc), F, out);
            }
            free(row);
        }
        free(tw), free(ta), free(pa), free(v), free(tmp), free(y), free(sign), free(src), free(wire);
        cases++;
    }
    fclose(in);
    if (fclose(out)) return 3;
    printf("ofdmmod law ok: %d cases\n", cases);
    return 0;
}
