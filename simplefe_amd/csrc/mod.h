// mod.h -- what mod.hip (the kernel) and api_mod.hip (the handle and the law's host twin) share: the limits of a shape,
// the tile, the arguments of a launch and the launcher.  No kernels here.
#pragma once
#include "common.h"
#include "vit.h"

namespace sfe {

constexpr int MOD_MAX_PRE = 4096, MOD_MAX_SPS = 64, MOD_MAX_ARM = 64;      // preamble symbols, samples per symbol, taps per arm (Q)
constexpr int MOD_MAX_TAPS = MOD_MAX_ARM * MOD_MAX_SPS;
constexpr int MOD_TABLE = 4 * VIT_MAX_PERIOD;                               // kept positions of one puncturing period at most

// A workgroup of MOD_THREADS threads writes one tile of MOD_TILE consecutive samples of the output stream, a thread two
// neighbouring samples at a time.  Its LDS: the taps, zero-filled up to Q sps, and the symbols the tile's samples read --
// at most MOD_TILE + MOD_MAX_ARM of them (sps = 1; fewer at every larger sps) -- as float2.
constexpr int MOD_THREADS = 256, MOD_TILE = 1024;
constexpr int MOD_TILE_SYMS = MOD_TILE + MOD_MAX_ARM;
constexpr size_t MOD_LDS_BYTES = (size_t)MOD_MAX_TAPS * 4 + (size_t)MOD_TILE_SYMS * 8;

// Everything a call needs travels by value, but the two tables a handle owns on the device: the taps and the
// amp-scaled preamble.  Nothing a handle holds changes after create.
struct ModArgs {
    const uint8_t *bytes;       // burst b's payload at bytes + b in_stride
    void *out;                  // n_out cf32 samples, or (n_out / 2) 5-byte groups
    const float *taps;          // [n_taps]
    const v2f *pre;             // [Lp], already scaled by amp
    long long in_stride, start_base, start_step, n_out, n_bursts;
    // the grid: n_lead tiles of zeros before the first frame, then tiles_per_slot tiles for each burst's slot
    // [o_b, o_b + start_step) -- the last burst's ends with its frame -- then the tiles of zeros behind the last frame
    long long n_lead, tiles_per_slot;
    unsigned gen[VIT_MAX_GEN];
    int K, n_gen, P, per_period, n_info, n_soft;    // n_gen = 0: uncoded
    int order, Lp, N, sps, n_taps, Q, F, tx10;
    float a;                    // a data symbol's component: amp (BPSK), float32(amp / sqrt 2) (QPSK)
    uint8_t pos[MOD_TABLE];     // kept position i of a period: (t mod P) << 2 | j
};

// One call: one launch over every tile of the stream.  Shapes and buffers are the caller's (api_mod.hip) to check.
int launch_mod(const ModArgs &a, long long n_tiles, hipStream_t st);

}  // namespace sfe
