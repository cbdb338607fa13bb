// fsk.h -- what fsk.hip (the kernels) and api_fsk.hip (the handle and the host plan) share: the tiles, the LDS of a
// workgroup, the arguments of a launch and the launchers.  The law is fsk_law.h's.  No kernels here.
#pragma once
#include "common.h"
#include "fsk_law.h"

namespace sfe {

// ---- modulator: a workgroup of FSK_THREADS threads writes one tile of FSK_TILE consecutive samples of the output stream (the
// tiles are cut as mod.hip cuts them).  Its LDS: the table C[0 .. n_taps], the levels of the symbols in flight anywhere in
// the tile and the prefix sums of those levels -- at most FSK_TILE / FSK_MIN_SPS + FSK_MAX_ARM + 2 symbols, the successor
// sample of a TX10 group included -- and the four waves' partial counts, each array on a 16-byte boundary.
constexpr int FSK_THREADS = 256, FSK_TILE = 1024;
constexpr int FSK_TILE_SYMS = FSK_TILE / FSK_MIN_SPS + FSK_MAX_ARM + 2;
constexpr size_t fsk_r16(size_t bytes) { return (bytes + 15) / 16 * 16; }
constexpr size_t FSK_MOD_LDS_BYTES = fsk_r16(((size_t)FSK_MAX_TAPS + 1) * 4) + fsk_r16((size_t)FSK_TILE_SYMS * 4) +
                                     fsk_r16(((size_t)FSK_TILE_SYMS + 1) * 4) + 4 * 4;        // 21056

struct FskModArgs {
    const uint8_t *bytes;       // burst b's payload at bytes + b in_stride
    void *out;                  // n_out cf32 samples, or (n_out / 2) 5-byte groups
    const uint32_t *C;          // [n_taps + 1], the handle's
    const uint8_t *pre;         // [ceil(Lp / 8)] packed MSB-first, pad bits 0, the handle's
    long long in_stride, start_base, start_step, n_out, n_bursts;
    long long n_lead, tiles_per_slot;       // the grid, as ModArgs'
    uint32_t Gsum;
    int Lp, N, sps, n_taps, F;
    float amp;
};

// ---- demodulator: one workgroup per burst.  Its LDS: two trees of FSK_TREE_WORDS floats (S1 and Se of as many timing
// candidates at a time as fit: FSK_TREE_WORDS / pow2(Lp), at least four), the nums and S1s of those candidates, and -- cf32
// input only, a byte is always finite -- the word of the non-finite flag.
constexpr int FSK_TREE_WORDS = 4096, FSK_MAX_CAND = 2 * FSK_MAX_RANGE + 1;
constexpr int FSK_CAND_WORDS = (FSK_MAX_CAND + 3) / 4 * 4;
constexpr size_t FSK_DEMOD_LDS_BYTES = 2 * (size_t)FSK_TREE_WORDS * 4 + 2 * (size_t)FSK_CAND_WORDS * 4 + 4;       // 33828; u8: 33824

struct FskDemodArgs {
    const void *in;             // stream s at in + s in_stride samples of the input format
    const unsigned *idx;        // or null: burst b of stream s at idx + s idx_stride + b
    const float *gate;          // or null: + s gate_stride + b
    const float *mf;            // [n_mf], the handle's
    const float *e;             // [Lp], the handle's
    float *soft;                // + (s n_bursts + b) soft_stride
    uint8_t *bits;              // or null: + (s n_bursts + b) bits_stride
    float *rec;                 // or null: + (s n_bursts + b) 8
    int *status;                // or null: + s status_stride + b
    long long in_stride, idx_stride, gate_stride, soft_stride, bits_stride, status_stride;
    long long n_in, n_bursts, start_base, start_step;
    float se, see, den, scale, min_gate;
    int sps, Lp, N, n_mf, delay, R;
};

int launch_fsk_mod(const FskModArgs &a, int tx10, long long n_tiles, hipStream_t st);
int launch_fsk_demod(const FskDemodArgs &a, int in_u8, int n_streams, hipStream_t st);

}  // namespace sfe
