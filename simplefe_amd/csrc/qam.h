// qam.h -- what qam.hip (the kernels) and api_qam.hip (the handle and the plan) share of the QAM mapper and soft demapper
// (sfe_dsp_qam_*): the tile of a workgroup, the arguments of a launch and the launchers.  The law itself is qam_law.h.
#pragma once
#include "common.h"
#include "qam_law.h"

namespace sfe {

constexpr int QAM_THREADS = 256;
constexpr unsigned QAM_TILE = 2048;         // symbols of one row a workgroup takes
constexpr unsigned QAM_GRID_X = 1u << 20;   // workgroups along x; the rest of a call's workgroups stack along y

// Everything a call needs travels by value, but the tables the handle owns on the device (perm, csi_index).
struct QamArgs {
    const void *in;             // map: row r's coded bytes at in + r in_stride; demap: its cf32 at in + r in_stride (cf32)
    void *out;                  // map: cf32 rows; demap: float rows
    const v2f *csi;             // demap on a handle with csi_period > 0: row r's channel at csi + r csi_stride
    const uint32_t *perm;       // [n_sym bps] or null
    const uint32_t *csi_index;  // [csi_period]
    long long in_stride, out_stride, csi_stride;
    unsigned n_sym, tiles, n_wg;        // tiles: workgroups per row; n_wg = tiles n_rows < 2^31
    unsigned csi_period;
    float scale;
    float lev[QAM_MAX_WORDS];
};

inline unsigned qam_tiles(size_t n_sym) { return (unsigned)((n_sym + QAM_TILE - 1) / QAM_TILE); }

// One call: one launch of a.n_wg workgroups.  Shapes and buffers are the caller's (api_qam.hip) to check.
int launch_qam_map(int bps, const QamArgs &a, hipStream_t st);
int launch_qam_demap(int bps, const QamArgs &a, hipStream_t st);

}  // namespace sfe
