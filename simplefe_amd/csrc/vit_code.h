// vit_code.h -- a validated convolutional code and its checker, shared by the Viterbi decoder's handle (api_vit.hip, where
// the checker is defined) and the burst modulator's (api_mod.hip).  HOST CODE ONLY; include it after host.h and vit.h.
#pragma once
#include "vit.h"

namespace sfe {

// a validated code, burst shape and input mode
struct VitCode {
    int K = 0, n = 0, P = 1, terminated = 1, n_info = 0, T = 0, n_soft = 0, per_period = 0, in_mode = 0, skip = 0;
    unsigned gen[VIT_MAX_GEN] = {0, 0, 0, 0};
    unsigned long long keep_lo = 0, keep_hi = 0;    // bit 4 (t mod P) + j: position (t, j) is transmitted

    int S() const { return vit_states(K); }
    bool kept(int tp, int j) const
    {
        const int bit = 4 * tp + j;
        return ((bit < 64 ? keep_lo : keep_hi) >> (bit & 63)) & 1ull;
    }
    unsigned label(unsigned reg) const          // bit j: coded bit c_j of the shift register reg
    {
        unsigned l = 0;
        for (int j = 0; j < n; j++) l |= (unsigned)(__builtin_popcount(reg & gen[j]) & 1) << j;
        return l;
    }
    // floats per burst row element, and where soft value i lies: the float at in_off() + i in_mul()
    int elem_floats() const { return in_mode == SFE_VIT_IN_SOFT ? 1 : 2; }
    int in_off() const { return in_mode == SFE_VIT_IN_SOFT ? 0 : 2 * skip; }
    int in_mul() const { return in_mode == SFE_VIT_IN_BPSK ? 2 : 1; }
    // elements of the mode's type a burst's row must hold
    size_t row_elems() const
    {
        if (in_mode == SFE_VIT_IN_SOFT) return (size_t)n_soft;
        return (size_t)skip + (in_mode == SFE_VIT_IN_BPSK ? (size_t)n_soft : ((size_t)n_soft + 1) / 2);
    }
};

// the code alone (K, generators, puncturing, ending, n_info): SFE_OK and *c filled in, or SFE_EINVAL with a message that
// starts with `who`
int vit_check_code(const char *who, int K, int n_gen, const uint32_t *gen, const uint8_t *keep, int P, int terminated, size_t n_info, VitCode *c);

}  // namespace sfe
