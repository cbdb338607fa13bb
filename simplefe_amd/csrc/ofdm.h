// ofdm.h -- what ofdm.hip (the kernel) and api_ofdm.hip (the handle and its float64 twin) share: the limits of a shape,
// the LDS layout of a burst, the statuses and the launcher.  No kernels here.
#pragma once
#include "common.h"

namespace sfe {

constexpr int OFDM_MIN_LOGN = 6, OFDM_MAX_LOGN = 12, OFDM_MAX_TRAIN = 4, OFDM_MAX_DATA = 4096;
constexpr int OFDM_OK = 0, OFDM_NO_ESTIMATE = 1, OFDM_GATED = 2, OFDM_OUT_OF_RANGE = 3;
constexpr int OFDM_NULL = 0, OFDM_DATA = 1, OFDM_PILOT = 2;    // kind[k]
constexpr int OFDM_REC = 8;         // float32 words of a record: eps, h2, min |H|^2 / h2, pilot error, arg phi_0, arg phi_last, +0, +0

// One workgroup per burst: a quarter of N lanes, at least one wave and at most four, so that every lane has a radix-4
// butterfly in every pass from N = 256 on and N = 64 costs one wave, whose barriers are free.
constexpr int ofdm_threads(int logn) { return (1 << logn) / 4 < 64 ? 64 : ((1 << logn) / 4 > 256 ? 256 : (1 << logn) / 4); }
// LDS of one burst: the transform's N cf32, H as N cf32, and the partial sums of the waves.  N = 4096: 65 664 bytes,
// two workgroups on a compute unit's 160 KiB.
constexpr int OFDM_RED_WORDS = 4 * 8;
constexpr size_t ofdm_lds_bytes(int logn) { return ((size_t)2 << logn) * 8 + OFDM_RED_WORDS * 4; }

struct OfdmArgs {
    const void *in;             // stream s at in + s in_stride samples of the input format
    const unsigned *idx;        // or null: burst b of stream s at idx + s idx_stride + b
    const float *gate;          // or null: + s gate_stride + b
    const v2f *tw;              // [N]: exp(-j 2 pi q / N)
    const v2f *c;               // [N]: conj(train) / (T |train|^2) on used bins, +0 elsewhere
    const v2f *pilot;           // [N]
    const float *sign;          // [Ns]: +-1
    const int *bins;            // [Nu]: the Nd data bins in increasing k, then the Np pilot bins in increasing k
    v2f *out;                   // + (s n_bursts + b) out_stride
    v2f *chan;                  // or null: + (s n_bursts + b) N
    float *rec;                 // or null: + (s n_bursts + b) 8
    int *status;                // or null: + s status_stride + b
    long long in_stride, idx_stride, gate_stride, out_stride, status_stride;
    long long n_in, n_bursts, start_base, start_step;
    float min_gate, nu, pilot_den;          // Nu, and Ns sum_pilot |pilot|^2 formed in float64 and rounded once
    int logn, cp, g, T, Ns, Nd, Np, cfo, q, mrc;
};

// the launch's LDS, where the default limit of a launch does not hold it; once per handle, on its device
int ofdm_prepare(int logn);
// One call: n_streams * n_bursts >= 1 workgroups.  Shapes and buffers are the caller's (api_ofdm.hip) to check.
int launch_ofdm(const OfdmArgs &a, int in_u8, int n_streams, hipStream_t st);

}  // namespace sfe
