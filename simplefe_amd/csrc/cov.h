// cov.h -- what cov.hip (the kernels) and api_cov.hip (the handle) share: the chunk length of the summation order, the
// limits of a shape, and the order in which the kernels keep a band's Gram matrix.  Plain C++: no kernels here.
#pragma once
#include "common.h"

namespace sfe {

constexpr int COV_T = 64;               // instants per chunk: sixteen K-steps of v_mfma_f32_16x16x4_f32
constexpr int COV_MAX_IN = 64, COV_MAX_BANDS = 1024;
constexpr int COV_MAX_AVG = 1 << 24;

// The 2S rows of U go in NT tiles of 16; only the tiles (I, J) with I <= J are computed, numbered row by row:
// (0,0) (0,1) .. (0,NT-1) (1,1) ..
inline int cov_nt(int S) { return (2 * S + 15) / 16; }
inline int cov_tiles(int S) { return cov_nt(S) * (cov_nt(S) + 1) / 2; }
// Floats of one band's sums in fragment order, [tile][64 lanes][4]: lane l, register r of tile (I, J) is
// G[16 I + 4 (l >> 4) + r][16 J + (l & 15)].  The carried sums and the scratch of group sums are kept in it.
inline size_t cov_frag_floats(int S) { return (size_t)cov_tiles(S) * 256; }

// The group pieces of a call that starts j0 chunks into a row (j0 < AC, the chunks per row) and completes q >= 1
// chunks; *rows = the rows it touches.  The host sizes the scratch ([M][pieces][cov_frag_floats] floats; none when a
// chunk is a whole row) and the grids with it.
long long cov_pieces(long long j0, long long q, int AC, int C, long long *rows);

// One call: q = n_in / COV_T chunks of every band, then the row folds.  Shapes and buffers are the caller's
// (api_cov.hip) to check: 1 <= S <= 64, 1 <= M <= 1024, j0 < AC, n_in = q COV_T > 0, scratch of cov_pieces() group sums.
int launch_cov(int u8, const void *in, long long in_stride, const float *group_in, float *group_out, const float *row_in,
               float *row_out, float *scratch, float *out, long long out_stride, long long n_in, int S, int M, int AC, int C,
               long long j0, float scale, hipStream_t st);

}  // namespace sfe
