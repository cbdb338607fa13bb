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

// ---- the store path of a pair of neighbouring samples i0, i0 + 1 of the stream, shared with fsk.hip.  cf32: 16 bytes where
// the pair's address allows it, else two 8-byte stores; `two` false: y0 alone.  TX10: i0 is even and the pair is one 5-byte
// group of the stream, quantised as sfe_dsp_tx_f32_to_10bit does.
__device__ __forceinline__ unsigned mod_q10(float x) { return (unsigned)((int)(short)(int)(x * 511.0f) + 512) & 0x3FFu; }

template <bool TX10>
__device__ __forceinline__ void mod_store_pair(void *out, long long i0, v2f y0, v2f y1, bool two)
{
    if (TX10) {
        const unsigned u0 = mod_q10(y0.x), u1 = mod_q10(y0.y), u2 = mod_q10(y1.x), u3 = mod_q10(y1.y);
        const unsigned w = ((u0 >> 8) | ((u1 >> 8) << 2) | ((u2 >> 8) << 4) | ((u3 >> 8) << 6)) | ((u0 & 0xFFu) << 8) |
                           ((u1 & 0xFFu) << 16) | ((u2 & 0xFFu) << 24);
        unsigned char *p = static_cast<unsigned char *>(out) + (i0 >> 1) * 5;
        __builtin_memcpy(p, &w, 4);
        p[4] = (unsigned char)u3;
    } else {
        v2f *p = static_cast<v2f *>(out) + i0;
        if (!two) {
            p[0] = y0;
        } else if ((reinterpret_cast<uintptr_t>(p) & 15) == 0) {
            *reinterpret_cast<v4f *>(p) = v4f{y0.x, y0.y, y1.x, y1.y};
        } else {
            p[0] = y0;
            p[1] = y1;
        }
    }
}

// One call: one launch over every tile of the stream.  Shapes and buffers are the caller's (api_mod.hip) to check.
int launch_mod(const ModArgs &a, long long n_tiles, hipStream_t st);

}  // namespace sfe
