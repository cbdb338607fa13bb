// beam_view.h -- what sfe_dsp_mvdr_load_beam (api_mvdr.hip) may see of a beamformer handle (api_beam.hip): its shape,
// its device and the fragment table its kernels read.  HOST CODE ONLY, like host.h and block.h.
#pragma once

namespace sfe {

struct BeamView {
    int S, B, M, device;
    float *frag;                // [M][beam_frag_floats(S, B)], owned by the handle
};

// false (message set by the handle cast, none for a null handle) unless h is a live beamformer handle
bool beam_view(void *h, BeamView *out);

}  // namespace sfe
