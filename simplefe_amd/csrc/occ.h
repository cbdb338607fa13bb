// occ.h -- what occ.hip (the kernel) and api_occ.hip (the handle) share of the spectrum occupancy detector (sfe_dsp_occ_*).
// The law itself is occ_law.h.
#pragma once
#include "common.h"
#include "occ_law.h"

namespace sfe {

struct OccArgs {
    const float   *in;          // row j of stream s at in + s*in_stride + j*n floats
    sfe_occ_info  *info;        // slot q = s*out_stride + j of each output
    sfe_occ_rec   *rec;
    unsigned char *mask;        // or null
    long long      in_stride, out_stride;
    unsigned       n_rows;      // per stream; n_streams * n_rows is 1 .. 2^31 - 1
    OccParams      p;
};
// One launch: a workgroup per row.  The buffers and the parameters are the caller's (api_occ.hip) to check.
int launch_occ(const OccArgs &a, unsigned n_streams, hipStream_t st);

}  // namespace sfe
