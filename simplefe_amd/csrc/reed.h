// reed.h -- what reed.hip (the kernels) and api_reed.hip (the handle) share of the Reed-Solomon outer code (sfe_dsp_reed_*).
// The law itself is reed_law.h.
#pragma once
#include "common.h"
#include "reed_law.h"

namespace sfe {

// The handle's tables on the device, one allocation of bytes:
//   [0, 64) roots   [64, 128) generator coefficients gen[0 .. n_par)   [128, 384) z_j   [384, 640) X_j^(1 - fcr)
//   [640, 640 + 4096) the whitening bytes, zero behind the frame
//   then four copies of them as dwords, copy h starting at byte h: a row read in aligned dwords from h bytes into the frame
//   on meets its whitening in aligned dwords too
constexpr int REED_TAB_ROOT = 0, REED_TAB_GEN = 64, REED_TAB_ZINV = 128, REED_TAB_XF = 384, REED_TAB_WHITEN = 640;
constexpr int REED_WHITEN_ROW = 4096, REED_TAB_WHITEN4 = REED_TAB_WHITEN + REED_WHITEN_ROW;
constexpr int REED_TAB_BYTES = REED_TAB_WHITEN4 + 4 * REED_WHITEN_ROW;
constexpr int REED_WAVES = 4;               // waves of a workgroup, a codeword each at a time
constexpr int REED_ROW = 260;               // bytes between the codewords of a workgroup in LDS: 256 and one bank on
constexpr int REED_ROWS = 16;               // codewords a workgroup holds: one frame of depth >= 4, or 4 / depth frames

struct ReedArgs {
    const uint8_t *in;          // frame (decode) or payload (encode) b at in + b*in_stride
    const int     *status_in;   // decode: or null
    uint8_t       *out;         // payload (decode) or frame (encode) b at out + b*out_stride
    uint32_t      *rec;         // decode: or null
    int           *status;      // decode: or null
    const uint8_t *tab;
    long long      in_stride, out_stride, n_frames;
    int            prim, n, n_par, k, t, depth;
    int            fpb;         // frames a workgroup takes: max(1, 4 / depth)
    unsigned       recip;       // ceil(2^16 / depth): floor(q / depth) = q * recip >> 16 for q < 4096
    int            whiten;      // the tables hold a whitening sequence
};
// One launch each.  The buffers and the shape are the caller's (api_reed.hip) to check.
int launch_reed_decode(const ReedArgs &a, hipStream_t st);
int launch_reed_encode(const ReedArgs &a, hipStream_t st);

}  // namespace sfe
