// ofdmmod.h -- what ofdmmod.hip (the kernel) and api_ofdmmod.hip (the handle and the plan) share: the grid of a call, the
// arguments of a launch and the launcher.  The law itself is ofdmmod_law.h.  No kernels here.
#pragma once
#include "common.h"
#include "ofdm.h"
#include "ofdmmod_law.h"

namespace sfe {

// A symbol is one workgroup of ofdm_threads(log2 N) lanes (ofdm.h) over N cf32 of LDS; the samples in no frame are cut
// into tiles of OFDMMOD_ZTILE samples, a workgroup of the same size each.
constexpr int OFDMMOD_ZTILE = 4096;
constexpr size_t ofdmmod_lds_bytes(int logn) { return ((size_t)1 << logn) * 8; }

// Everything a call needs travels by value, but the tables the handle owns on the device (law).
struct OfdmmodArgs {
    OmodLaw law;
    const void *in;             // burst b's row at in + b in_stride: bytes (BITS mode) or cf32 (SYMBOLS mode)
    void *out;                  // n_out cf32 samples, or (n_out / 2) 5-byte groups
    long long in_stride, start_base, start_step, n_out, n_bursts;
    // the grid: n_lead tiles of zeros before the first frame; then per burst T + Ns symbol workgroups and gap_tiles tiles
    // of the zeros between its frame and the next (the last burst's leave at once); then the tiles behind the last frame
    long long n_lead, gap_tiles;
    int F, tx10;
};

// One call: one launch of n_wg workgroups.  Shapes and buffers are the caller's (api_ofdmmod.hip) to check.
int launch_ofdmmod(const OfdmmodArgs &a, long long n_wg, hipStream_t st);

}  // namespace sfe
