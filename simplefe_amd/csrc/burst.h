// burst.h -- what burst.hip (the kernel) and api_burst.hip (the handle and its float64 twin) share: the limits of a shape,
// the LDS layout of a burst, the statuses and the launcher.  No kernels here.
#pragma once
#include "common.h"
#include "eig.h"

namespace sfe {

constexpr int BURST_MIN_SPS = 4, BURST_MAX_SPS = 64, BURST_MIN_SYM = 2, BURST_MAX_SYM = 4096;
constexpr int BURST_OK = 0, BURST_NO_ESTIMATE = 1, BURST_GATED = 2, BURST_OUT_OF_RANGE = 3;
constexpr int BURST_REC = 8;        // float32 words of a record: tau, f, theta, a, q, evm, +0, +0

// LDS of one burst: y [N] and z [Lp] as cf32, the table of sps twiddles [64], the partial sums of the four waves, and --
// where it fits the budget -- the reach of (N + 2) sps samples.  Step 2 of the law has lane k read samples k sps + const:
// eight-byte reads, whose bank pair is the slot mod 32 within a half-wave of 32 lanes, so an even sps would put the lanes
// on 32 / gcd(sps, 32) pairs only (sps = 4: 4-way conflicts, 32 and 64: 32-way).  Sample i of symbol period s = i / sps
// therefore sits in slot i + s * pad, pad = 1 for an even sps and 0 for an odd one: the lanes are then an odd number of
// slots apart, on 32 different pairs for every sps.
constexpr int BURST_RED_WORDS = 4 * 4;
constexpr size_t BURST_LDS_BUDGET = eig_lds_bytes(EIG_MAX_IN, 1);       // what the eigen-solver already asks of a launch
constexpr size_t burst_reach(int sps, int N) { return ((size_t)N + 2) * (size_t)sps; }
__host__ __device__ constexpr int burst_pad(int sps) { return (sps & 1) ^ 1; }
constexpr size_t burst_base_bytes(int N, int Lp) { return ((size_t)N + (size_t)Lp + BURST_MAX_SPS) * 8 + BURST_RED_WORDS * 4; }
constexpr size_t burst_stage_bytes(int sps, int N) { return (burst_reach(sps, N) + ((size_t)N + 2) * burst_pad(sps)) * 8; }
constexpr bool burst_staged(int sps, int N, int Lp) { return burst_base_bytes(N, Lp) + burst_stage_bytes(sps, N) <= BURST_LDS_BUDGET; }

struct BurstArgs {
    const void *in;             // stream s at in + s in_stride samples of the input format
    const unsigned *idx;        // or null: burst b of stream s at idx + s idx_stride + b
    const float *gate;          // or null: + s gate_stride + b
    const v2f *pre;             // [Lp]
    const v2f *tw;              // [sps]: exp(-j 2 pi r / sps)
    v2f *out;                   // + (s n_bursts + b) out_stride
    float *rec;                 // or null: + (s n_bursts + b) 8
    int *status;                // or null: + s status_stride + b
    long long in_stride, idx_stride, gate_stride, out_stride, status_stride;
    long long n_in, n_bursts, start_base, start_step;
    float E_p, min_gate;
    int sps, N, Lp, lag, fixed_timing, staged;
};

// One call: n_streams * n_bursts >= 1 workgroups.  Shapes and buffers are the caller's (api_burst.hip) to check.
int launch_burst(const BurstArgs &a, int in_u8, int n_streams, hipStream_t st);

}  // namespace sfe
