// mvdr.h -- what mvdr.hip (the kernels) and api_mvdr.hip (the handle) share: the limits of a shape, the LDS layout of a
// problem and the launchers.  Plain C++: no kernels here.
#pragma once
#include "common.h"

namespace sfe {

constexpr int MVDR_MAX_IN = 64, MVDR_MAX_BEAMS = 64, MVDR_MAX_BANDS = 1024;      // the beamformer's own limits (beam.h)
constexpr long long MVDR_MAX_WEIGHTS = 1LL << 20;                                 // M B S
constexpr int MVDR_MAX_N = 2 * MVDR_MAX_IN;                                       // n = 2S, the order of a problem
// The factor lives in LDS as a packed lower triangle, row-major: L[i][j], j <= i, at i (i + 1) / 2 + j.
constexpr int MVDR_TRI = MVDR_MAX_N * (MVDR_MAX_N + 1) / 2;                       // 8256 floats, 33 024 bytes
// Right-hand sides go through in passes of MVDR_SLOTS: eight per wave, each shared by eight lanes.
constexpr int MVDR_SLOTS = 32;

struct MvdrArgs {
    const float *gram;          // row j of band k at gram + k in_stride + j n^2
    const float *steer;         // [M][B][S] (re, im)
    const float *fallback;      // [M][2B][2S]: the conventional beamformer's real matrix
    float *R;                   // row j, band k at R + j out_stride + k 4BS
    float *power;               // or null: + j power_stride + k B + b
    int *status;                // or null: + j status_stride + k
    long long in_stride, out_stride, power_stride, status_stride;
    int S, B, M;
    float load_rel, load_abs;
};

// One call: n_rows >= 1 rows of every band, one workgroup per (row, band).  Shapes and buffers are the caller's
// (api_mvdr.hip) to check.
int launch_mvdr(const MvdrArgs &a, int widely_linear, long long n_rows, hipStream_t st);

// frag[k][beam_frag_floats(S, B)] = R[k][2B][2S] in the beamformer's fragment order (beam.h: beam_frag_at), padding zero.
int launch_mvdr_load_beam(const float *R, float *frag, int S, int B, int M, hipStream_t st);

}  // namespace sfe
