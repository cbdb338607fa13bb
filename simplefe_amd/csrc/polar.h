// polar.h -- what polar.hip (the kernel) and api_polar.hip (the handle) share of the FM, phase and envelope detector
// (sfe_dsp_polar_*).  The law itself is polar_law.h.
#pragma once
#include "common.h"

namespace sfe {

constexpr int POLAR_MAX_STREAMS = 32767;    // grid.y

struct PolarArgs {
    const void *in;             // stream 0's samples: cf32, or (I,Q) byte pairs
    float      *out;
    const v2f  *state_cur;      // [n_streams] x[-1] of this call (FM reads it)
    v2f        *state_nxt;      // [n_streams] x[n_in - 1] as float32 (FM writes it)
    long long   in_stride, out_stride;      // samples
    unsigned    n_in;           // 1 .. 2^31 - 1
    float       gain;
};
// One launch: tiles x n_streams workgroups.  The buffers are the caller's (api_polar.hip) to check: element alignment, strides
// that cover n_in, 1 <= n_streams <= POLAR_MAX_STREAMS.
int launch_polar(int mode, int in_u8, const PolarArgs &a, int n_streams, hipStream_t st);

}  // namespace sfe
