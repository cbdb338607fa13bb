// iir.h -- what iir.hip (the kernels) and api_iir.hip (the handle) share: the limits and the table layout of the
// biquad-cascade IIR filter (sfe_dsp_iir_*).
#pragma once
#include "common.h"

namespace sfe {

constexpr int IIR_MAX_SECTIONS = 8;
// floats of one section's constants: 5 coefficients (+3 of padding), 7 matrices A^(16 2^k), 16 correction rows
// [1 0] A^k, 64 matrices A^(16 l) -- struct IirSec in iir.hip
constexpr int IIR_SEC_FLOATS = 8 + 7 * 4 + 16 * 2 + 64 * 4;

int iir_block();                // G: samples per block, the granule of a call
int iir_group();                // K: blocks per group of the two-level fold
int iir_groups(long long B0, int nb);
int launch_iir(int fmt, const void *in, long long in_stride, void *out, long long out_stride, const void *sec, const float *phi,
               const float *phik, float *table, const float *state_cur, float *state_nxt, long long B0, int nb, int S, int n_streams,
               hipStream_t st);

}  // namespace sfe
