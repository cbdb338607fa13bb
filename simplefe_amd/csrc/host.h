// host.h -- what the host-side translation units of libsfe_dsp.so share: the handles behind sfe_fir_t / sfe_rs_t,
// the plan caches, and the helpers that cross files.  HOST CODE ONLY (no kernels; not part of the kernel-source hash).
//   api.hip          errors, devices, memory, timers, the synthetic stream, the wire-format converters
//   api_plans.hip    folding (U, step, pos0) into the polyphase kernels' tap tables and spectra
//   api_fir.hip      the FIR handle: upload of the tables, variants, the host round trips, sfe_dsp_fir_*
//   fir_plan.h       what api_fir.hip works out before it uploads or launches, without HIP: the tap partitions, the single-transform
//                    overlap, the spectrum tables and twiddle bases, the variant key's size class (included below;
//                    tests/host/test_fir_plan.cpp); api_rs.hip builds the general-rate kernel's tables from it too
//   api_rs.hip       the resample / decimate handle: a call's checks, kernel choice, plan upload, carried state, sfe_dsp_rs_*
//   rs_plan.h        what api_rs.hip works out before it launches, without HIP: the integer-step closed form, the general-rate
//                    plan and its run memo, the walks over a plan (included below; tests/host/test_rs_plan.cpp)
//   api_pipe.hip     the pinned host pipe over either handle, sfe_dsp_*_pipe_*
//   group.hip        channel blocks over several devices, sfe_dsp_*_group_* (over the public C ABI only)
//   block.h          what every handle is built from: owners of device and pinned memory (grow-only ones too), streams and events,
//                    the carried pair, the history epilogue and load_history of the two handles here, create's device scope, the
//                    handle cast, process_stream's refusals (call_checks.h) (included below)
//   api_<block>.hip  the streaming blocks over block.h: chan, combine, ddc, psd, corr, iir, beam, cov, mvdr, eig, burst, vit, mod
#pragma once
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <map>
#include <mutex>
#include <new>
#include <tuple>
#include <numeric>
#include <unordered_map>
#include <utility>
#include <vector>

#include "common.h"
#include "block.h"
#include "fir_plan.h"
#include "rs_plan.h"
#include "segtile.h"
#include "timelaw.h"

namespace sfe {

static_assert(FIR_PLAN_N == FFT_N, "fir_plan.h plans for the kernels' transform length");

// ---- plan caches (api_plans.hip): (step, pos0) -> the plan the kernels read (common.h: raw pointers) beside the owners of
// its N device tables; a plan without tables marks a shape that has no such kernel
template <class Plan, int N>
struct PlanEntry {
    Plan plan;
    DevBuf<float> d[N];
};
template <class Plan, int N> using PlanMap = std::map<std::pair<int, long long>, PlanEntry<Plan, N>>;
using PlanCache = PlanMap<PolyTiledPlan, 2>;
using FftPlanCache = PlanMap<PolyFftPlan, 2>;
using MfmaCache = PlanMap<PolyMfmaPlan, 1>;
// nullptr: the shape has no such kernel (the caller takes the next one); *rc != SFE_OK: the upload failed
const PolyTiledPlan *get_tiled_plan(PlanCache &cache, const std::vector<float> &taps_pm, int U, int plen, int step, long long pos0,
                                    int *rc);
const PolyFftPlan *get_fft_plan(FftPlanCache &cache, const std::vector<float> &taps_pm, int U, int plen, int step, long long pos0,
                                int fft_mode, int *rc);
const PolyMfmaPlan *get_mfma_plan(MfmaCache &cache, const std::vector<float> &taps_pm, int U, int plen, int step, long long pos0,
                                  int *rc);

// ---- the FIR handle (api_fir.hip)
struct FirTables {              // fir_plan.h's spectra and twiddle bases on the device: replaced as a whole by a re-plan
    DevBuf<v2f> hs, tw1, tw2;
    int upload(const FirShape &sh, const float *taps);
};
struct FirStage {               // sfe_dsp_fir_process_host: chunked pinned + device staging, made by its first call
    PinnedBuf<char> h, h_out;
    DevBuf<char> d_in, d_out;
};
struct Fir {
    static constexpr uint32_t MAGIC = 0x46495231u;   // 'FIR1': catches stale or foreign handles
    uint32_t magic = MAGIC;
    int n_taps = 0, taps_complex = 0, data_complex = 0, out_complex = 0, n_channels = 1;
    int device = 0, algo = SFE_FIR_ALGO_AUTO, in_u8 = 0, out_tx10 = 0;
    int blk = 0, block_hint = 0;
    int hl = 0;                 // carried history per channel, samples (multiple of 256)
    int ovl = 0;                // overlap of one transform (multiple of 256): each launch applies `ovl` (+1) taps
    int variant = FIR_VAR_AUTO; // data movement of the cf32 kernel: measured per device and shape unless sfe_dsp_fir_set_variant fixed it
    int last_variant = FIR_VAR_AUTO, cal_runs = 0;      // what the last bulk call ran; calibrations this handle made
    float cal_ms[FIR_VAR_COUNT] = {0.0f, 0.0f, 0.0f};   // medians of this handle's last calibration, by variant
    int piped = 0;              // pipes alive over this handle: they froze its item formats, so the format setters refuse
    int per_channel = 0;        // taps given per channel ([n_channels][n_taps]): one spectrum set per channel
    int parts = 1;              // partitions of the tap vector, one launch each (filters longer than one overlap)
    bool fft_ok = false;
    Stream stream;              // (first of the owners: destroyed after the buffers)
    FirTables tab;
    DevBuf<unsigned> ticket;    // work counters of the persistent FFT kernel (zero between launches)
    DevBuf<float> d_taps;       // real taps for the direct kernel
    std::vector<float> h_taps;  // host copy (direct-kernel plan)
    std::vector<float> h_taps_all;   // every tap as given at create (complex pairs / per-channel rows included): re-planning
    PlanCache plans;
    CarriedPair hist;
    bool captured = false;      // a call of this handle sits in a hipGraph that names hist.cur(): the state stays there (fir_run)
    bool started = false;       // samples have gone through since create / reset
    // class-compatible host block path
    PinnedBuf<float> h_buf;     // block_hint+2 floats (blkconv.cxx:44 sizes it so)
    DevBuf<char> d_blk_in, d_blk_out;
    PinnedBuf<char> h_blk_out;  // the kernel's output of a zero-copy block (then copied over h_buf)
    FirStage stage;
    // Calls of at most zc_max samples skip the two DMA copies: the kernel reads the pinned host buffer
    // and writes a pinned host buffer itself (one launch + one wait instead of copy, launch, copy, wait).
    // Only where the kernel reads its input once (parts == 1).  sfe_dsp_fir_set_zero_copy_max; 0 disables.
    size_t zc_max = (size_t)1 << 20;
    size_t hist_bytes() const { return (size_t)n_channels * hl * (data_complex ? 8 : 4); }
};
Fir *as_fir(void *h);
int fir_run(Fir *f, const void *d_in, void *d_out, size_t n, size_t in_stride, size_t out_stride, hipStream_t s);

// ---- the resample / decimate handle (api_rs.hip)
struct Rs {
    static constexpr uint32_t MAGIC = 0x52533031u;   // 'RS01'
    uint32_t magic = MAGIC;
    int U = 1, n_taps = 0, plen = 0, blksize = 0, data_complex = 0, n_channels = 1;
    int device = 0, mode = SFE_RS_RESAMPLE, exact_stream = 0, in_u8 = 0;
    int piped = 0;                         // pipes alive over this handle (they froze its input format)
    int fft_mode = 0;                      // sfe_dsp_rs_set_algo: 1 force the transform-domain kernel, -1 never, 0 the calibrated rule
    int use_mfma = 0;                      // sfe_dsp_rs_set_algo(SFE_RS_ALGO_MFMA): the matrix-pipe form (measured slower; opt-in)
    int hl = 0;
    Stream stream;                         // (first of the owners: destroyed after the buffers)
    DevBuf<float> d_taps;                  // [U][plen] phase-major
    std::vector<float> h_taps_pm;          // host copy of the same (tiled plans)
    PlanCache plans;
    MfmaCache mfma_plans;
    FftPlanCache fft_plans;
    DevBuf<unsigned> d_ticket;             // work counters of the transform-domain kernel
    FirTables gen_tables;                  // general rate in the transform domain (poly_gen.hip): the U phases' spectra and the
                                           // twiddle bases, from the FIR's own table builder (one tap set per phase); empty
    bool gen_tried = false;                // where a phase is longer than one transform overlaps, or until the first such call
    CarriedPair hist;
    bool captured = false;                 // a call of this handle sits in a hipGraph that names hist.cur() (see CarriedPair::carry)
    sfe_rs_timestate ts = {0, 0.0f, 0};
    // class-compatible host path staging (one channel); the grow-only ones (block.h: Grown) keep the policy of their caller
    DevBuf<char> d_in;
    Grown<DevBuf<char>> d_out;             // bytes
    struct Sched {                         // per-output schedule, (pos, mu): device arrays and their staging, one capacity
        Mirror<long long> pos;
        Mirror<float> mu;
        int grow(size_t n)
        {
            const int rc = pos.grow(n);
            return rc != SFE_OK ? rc : mu.grow(n);
        }
    };
    Grown<Sched> sched;
    Grown<PinnedBuf<char>> h_stage;        // in/out staging
    // wire-format input on a shape no fused u8 kernel takes (steps beyond the tiled kernels, a general rate outside the transform kernel):
    // the call's bytes are converted ONCE into this grow-only float32 buffer and the float path runs (api_rs.hip: sfe_dsp_rs_process_stream)
    Grown<DevBuf<float>> d_u8f;
    hipStream_t u8f_stream = nullptr;      // the caller's: borrowed
    bool u8_refused = false;               // set by the implementation where it would have refused a u8 call, nothing launched, no state touched
    Grown<Mirror<TlSeg>> segs;             // run-length plans: the memo's table, a launch's own runs behind it
    Grown<Mirror<SegChunk>> chunks;
    Event ev_plan;                         // recorded behind a call's plan uploads: the pinned staging is free again once it fires
    hipStream_t plan_stream = nullptr;     // ... on this stream, the caller's: borrowed (the device-side plan arrays are ordered by it)
    RsMemo memo;                           // general rate: the plans of the reference calls met so far, per start state (rs_plan.h)
    size_t seg_uploaded = 0;               // leading entries of memo.table already in segs->d (void once the memo is cleared or segs regrown)
    int esz() const { return data_complex ? 8 : 4; }
};
Rs *as_rs(void *h);

// where a call's samples lie, and the seven fields every polyphase kernel's arguments open with (common.h: Poly*Args);
// H: either handle
struct PolyIo {
    const void *in;
    void *out;
    long long n_in, in_stride, out_stride;
};
template <class A, class H>
void fill_io(A &a, const H *h, const PolyIo &io)
{
    a.in = io.in;
    a.out = io.out;
    a.hist = h->hist.cur();
    a.n_in = io.n_in;
    a.in_stride = io.in_stride;
    a.out_stride = io.out_stride;
    a.hl = h->hl;
}

// poly_rt_dma.hip (round 5): the runtime-shape tiled kernel for odd input steps, its tile fetched by LDS-DMA.  SFE_ESTATE: the shape or
// the buffers are outside what it takes -- the caller runs launch_poly_tiled.  (Declared here, not in common.h: host-side plumbing.)
int launch_poly_rt_dma(const PolyTiledPlan &plan, const PolyTiledArgs &a, int data_complex, int in_u8, int n_channels, hipStream_t s);
bool poly_rt_dma_window_shape(int SP, int UP);

}  // namespace sfe
