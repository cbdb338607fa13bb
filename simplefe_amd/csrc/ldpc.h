// ldpc.h -- what ldpc.hip (the kernels) and api_ldpc.hip (the handle and the host plan) share of the quasi-cyclic LDPC code
// (sfe_dsp_ldpc_*): the handle's table on the device, the LDS layout of a workgroup, and the launchers.  The law itself is
// ldpc_law.h.  No kernels here.
#pragma once
#include "common.h"
#include "ldpc_law.h"

namespace sfe {

constexpr int LDPC_THREADS = 256;                   // threads of a workgroup, both kernels
constexpr int LDPC_MAX_GROUP = 4;                   // codewords a decoding workgroup holds at most
constexpr int LDPC_CNT_WORDS = LDPC_MAX_ITER + 4;   // per word: unsatisfied checks after iteration 0 .. 64, then `bad`, then `flips`
constexpr int LDPC_CNT_BAD = LDPC_MAX_ITER + 1, LDPC_CNT_FLIPS = LDPC_MAX_ITER + 2;
constexpr size_t LDPC_SHARED_LDS = 65536;           // what several words of a workgroup may use together

// The handle's table on the device, uint32 words: [0, mb] the rows' first cells; from tab_cells on the cells, col | shift << 16;
// from tab_inv on (encodable codes) the blocks of the parity part's inverse, LdpcCode::inv.
//
// LDS of a decoding workgroup: the cells (4 bytes each), the mb + 1 row starts (4 bytes each), then per codeword
//   APP   int16 [n]      the running sums
//   L     int8  [n]      the quantised input, for the record's third word
//   msg   int8  [edges]  one message per edge, edge (cell q, row i) at q Z + i
//   cnt   uint32 [LDPC_CNT_WORDS]
// every part rounded up to 4 bytes.
struct LdpcLayout {
    int off_rows, off_words, off_L, off_msg, off_cnt, word_bytes, group, tpw;
    size_t lds;
};
constexpr int ldpc_up4(int v) { return (v + 3) & ~3; }
inline LdpcLayout ldpc_layout(int n, int n_cells, int mb, int Z)
{
    LdpcLayout l{};
    const int edges = n_cells * Z;
    l.off_rows = 4 * n_cells;
    l.off_words = (l.off_rows + 4 * (mb + 1) + 15) & ~15;
    l.off_L = ldpc_up4(2 * n);
    l.off_msg = l.off_L + ldpc_up4(n);
    l.off_cnt = l.off_msg + ldpc_up4(edges);
    l.word_bytes = (l.off_cnt + 4 * LDPC_CNT_WORDS + 15) & ~15;
    // a word's rows are walked by 256 / group threads: a whole wave or more, and no more words than 64 KB hold
    l.group = Z <= 64 ? 4 : (Z <= 128 ? 2 : 1);
    while (l.group > 1 && (size_t)l.off_words + (size_t)l.group * l.word_bytes > LDPC_SHARED_LDS) l.group /= 2;
    l.tpw = LDPC_THREADS / l.group;
    l.lds = (size_t)l.off_words + (size_t)l.group * l.word_bytes;
    return l;
}
// LDS of an encoding workgroup: the payload's bytes, mb doubled syndrome rows of enc_row_words(Z) words, the codeword's words
constexpr int ldpc_enc_row_words(int Z) { return (2 * Z + 31) / 32 + 2; }
inline size_t ldpc_enc_lds(int k_bytes, int n_bytes, int mb, int Z)
{
    return (size_t)ldpc_up4(k_bytes) + 4 * (size_t)mb * ldpc_enc_row_words(Z) + (size_t)ldpc_up4(n_bytes);
}

struct LdpcArgs {
    const float *in;            // decode: word b at in + b in_stride floats
    const uint8_t *payload;     // encode: word b at payload + b in_stride bytes
    const int *status_in;       // decode: or null
    uint8_t *out;               // decode: k_bytes at out + b out_stride; encode: n_bytes there
    uint32_t *rec;              // decode: or null: + 3 b
    int *status;                // decode: or null: + b
    const uint32_t *tab;
    long long in_stride, out_stride, n_words;
    int mb, Z, n, k, n_cells, tab_cells, tab_inv, Zw;
    int in_off, in_mul;         // soft value v is the float at in_off + v in_mul of the word's row
    float scale;
    int a, beta, max_iter;
    LdpcLayout lay;
};

// One launch each.  Shapes and buffers are the caller's (api_ldpc.hip) to check.  With prepare_only nothing is launched:
// the decoder is allowed its dynamic LDS on the current device, which create does once so that a call -- a captured one
// too -- is a launch and nothing else.
int launch_ldpc_decode(const LdpcArgs &a, hipStream_t st, bool prepare_only = false);
int launch_ldpc_encode(const LdpcArgs &a, hipStream_t st);

}  // namespace sfe
