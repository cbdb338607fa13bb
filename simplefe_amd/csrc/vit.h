// vit.h -- what vit.hip (the kernel) and api_vit.hip (the handle and the law's host twin) share: the limits of a code, the
// LDS layout of a burst, the statuses and the launcher.  No kernels here.
#pragma once
#include "common.h"
#include "burst.h"

namespace sfe {

constexpr int VIT_MIN_K = 3, VIT_MAX_K = 9, VIT_MIN_GEN = 2, VIT_MAX_GEN = 4, VIT_MAX_PERIOD = 32, VIT_MAX_INFO = 8192;
constexpr int VIT_OK = 0, VIT_NOT_FINITE = 1, VIT_UPSTREAM = 2;
constexpr uint32_t VIT_QNAN = 0x7fc00000u;      // the metric word of a burst without an answer
constexpr int VIT_MAX_WAVES = 4;                // bursts (waves) per workgroup at most

// LDS of one burst (one wave), every part a multiple of 8 bytes:
//   survivors  one 64-bit ballot word per 64 states and step: T * max(S, 64) / 8 bytes (a code of fewer than 64 states
//              still writes one word per step)
//   bits       the packed payload, ceil(n_info / 8) bytes rounded up to 8
//   soft       where it fits beside them: the T * n soft values, punctured positions filled in with +0
// A launch may ask for VIT_LDS_BUDGET, what the eigen-solver and the burst demodulator already ask for.  A burst whose
// three parts exceed it reads its soft values from global memory step by step; one whose survivors and bits alone
// exceed it (K = 9 beyond T = 4183 steps) is refused by create.
constexpr size_t VIT_LDS_BUDGET = BURST_LDS_BUDGET;
constexpr int vit_states(int K) { return 1 << (K - 1); }
constexpr int vit_words(int K) { return K <= 7 ? 1 : vit_states(K) / 64; }     // ballot words per step = states per lane
constexpr int vit_steps(int K, int terminated, int n_info) { return n_info + (terminated ? K - 1 : 0); }
constexpr size_t vit_surv_bytes(int K, int T) { return (size_t)T * vit_words(K) * 8; }
constexpr size_t vit_bits_bytes(int n_info) { return (((size_t)n_info + 7) / 8 + 7) / 8 * 8; }
constexpr size_t vit_soft_bytes(int n_gen, int T) { return ((size_t)T * n_gen * 4 + 7) / 8 * 8; }
constexpr size_t vit_base_bytes(int K, int T, int n_info) { return vit_surv_bytes(K, T) + vit_bits_bytes(n_info); }
constexpr bool vit_fits(int K, int T, int n_info) { return vit_base_bytes(K, T, n_info) <= VIT_LDS_BUDGET; }
constexpr bool vit_staged(int K, int n_gen, int T, int n_info) { return vit_base_bytes(K, T, n_info) + vit_soft_bytes(n_gen, T) <= VIT_LDS_BUDGET; }
constexpr size_t vit_burst_bytes(int K, int n_gen, int T, int n_info)
{
    return vit_base_bytes(K, T, n_info) + (vit_staged(K, n_gen, T, n_info) ? vit_soft_bytes(n_gen, T) : 0);
}
// bursts per workgroup: as many as the budget holds, VIT_MAX_WAVES at most
constexpr int vit_waves(int K, int n_gen, int T, int n_info)
{
    const size_t w = VIT_LDS_BUDGET / vit_burst_bytes(K, n_gen, T, n_info);
    return w >= (size_t)VIT_MAX_WAVES ? VIT_MAX_WAVES : (w < 1 ? 1 : (int)w);
}

// Everything a call needs travels by value: a handle owns no device memory, and nothing it holds changes after create.
struct VitArgs {
    const float *in;            // burst b at in + b in_stride floats
    const int *status_in;       // or null
    uint8_t *bits;              // + b out_stride bytes
    uint32_t *rec;              // or null: + 2 b
    int *status;                // or null: + b
    long long in_stride, out_stride, n_bursts;
    unsigned gen[VIT_MAX_GEN];
    unsigned long long keep_lo, keep_hi;    // bit 4 (t mod P) + j of the 128 set where position (t, j) is transmitted
    int K, n_gen, P, per_period, terminated, n_info, T, n_soft;
    int in_off, in_mul;         // soft value i is the float at in_off + i in_mul of the burst's row
    int staged, waves;
};

// One call: ceil(n_bursts / waves) workgroups of `waves` waves.  Shapes and buffers are the caller's (api_vit.hip) to check.
// With prepare_only nothing is launched: the kernel of the shape is allowed its dynamic LDS on the current device, which
// create does once so that a call -- a captured one too -- is a launch and nothing else.
int launch_vit(const VitArgs &a, hipStream_t st, bool prepare_only = false);

}  // namespace sfe
