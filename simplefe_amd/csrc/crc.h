// crc.h -- what crc.hip (the kernels) and api_crc.hip (the handle) share of the frame check (sfe_dsp_crc_*).  The law itself
// is crc_law.h.
#pragma once
#include "common.h"
#include "crc_law.h"

namespace sfe {

// Two launch classes.  Short rows: a wave per frame, CRC_SHORT_FPB frames per workgroup.  Long rows: a workgroup of
// CRC_LONG_T threads per frame.  A frame's whole dwords (in FRAME coordinates: dword d is bytes 4 d .. 4 d + 3 of the row,
// wherever the row starts) are dealt round robin over the T lanes of its group, T = 64 or CRC_LONG_T; up to 3 bytes stay behind.
constexpr int CRC_SHORT_MAX = 4096;         // payloads up to this many bytes take the short class
constexpr int CRC_SHORT_T = 64, CRC_SHORT_FPB = 4, CRC_LONG_T = 1024;

// The handle's constants on the device, uint32, all modulo G' (crc_law.h), made at create.  Per class of T lanes:
//   32 columns  x^(b + 32 T), b = 0 .. 31: the matrix that carries a lane's register over one round of T dwords
//   T weights   x^(32 (T - l)), l = 0 .. T - 1: what lane l's register is worth in the frame's
constexpr int CRC_TAB_SHORT = 0, CRC_TAB_LONG = 32 + CRC_SHORT_T, CRC_TAB_WORDS = CRC_TAB_LONG + 32 + CRC_LONG_T;

struct CrcArgs {
    const uint8_t  *in;         // payload (append) or channel frame (check) b at in + b*in_stride
    const int      *status_in;  // check: or null
    uint8_t        *out;        // frame (append) or payload (check) b at out + b*out_stride; check: or null
    uint32_t       *rec;        // check: or null
    int            *status;     // check: or null
    const uint8_t  *pn;         // the sequence, frame_bytes() bytes and zeros up to a multiple of 4 behind them; or null
    const uint32_t *tab;
    long long       in_stride, out_stride, n_frames;
    CrcLaw          law;
    uint32_t        init_term;  // initL x^(8 P) mod G': what a non-zero init adds to the register of a zero start
    int             check;
};
// One launch each.  The buffers and the shape are the caller's (api_crc.hip) to check.
int launch_crc(const CrcArgs &a, hipStream_t st);

}  // namespace sfe
