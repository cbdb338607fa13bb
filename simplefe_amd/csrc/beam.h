// beam.h -- what beam.hip (the kernels) and api_beam.hip (the handle) share: the padded shape classes and the order in
// which the kernel's lanes read a band's real matrix.  Plain C++: no kernels here.
#pragma once
#include "common.h"

namespace sfe {

constexpr int BEAM_MAX_IN = 64, BEAM_MAX_BEAMS = 64, BEAM_MAX_BANDS = 1024;
constexpr long long BEAM_MAX_WEIGHTS = 1LL << 20;       // M B S

// The class of a shape: KP pairs of MFMA K-steps (one pair takes four input streams: their real parts, then their
// imaginary parts) and RT tiles of 16 matrix rows (eight beams), each rounded up to a power of two.
inline int beam_kp(int S) { int k = 1; while (4 * k < S) k *= 2; return k; }
inline int beam_rt(int B) { int r = 1; while (8 * r < B) r *= 2; return r; }

// Floats of one band's matrix in fragment order: [RT][2 KP][64 lanes]
inline size_t beam_frag_floats(int S, int B) { return (size_t)beam_rt(B) * 2 * beam_kp(S) * 64; }

// Lane `lane` of K-step ks of row tile rt multiplies by R[row][col] (v_mfma_f32_16x16x4_f32: A[lane & 15][lane >> 4]);
// the entry is zero where row >= 2B or col >= 2S.
inline void beam_frag_at(int rt, int ks, int lane, int *row, int *col)
{
    *row = 16 * rt + (lane & 15);
    *col = 2 * (4 * (ks >> 1) + (lane >> 4)) + (ks & 1);
}

// One call: n_in >= 1 samples of M bands of S streams into B beams; frag holds M matrices of beam_frag_floats(S, B)
// floats.  Shapes and buffers are the caller's (api_beam.hip) to check.  u8: the input is (I,Q) byte pairs.
int launch_beam(int u8, const void *in, long long in_stride, v2f *out, long long out_stride, const float *frag, long long n_in,
                int S, int B, int M, hipStream_t st);

}  // namespace sfe
