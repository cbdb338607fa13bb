// api_fir.hip -- the FIR handle behind sfe_fir_t (blkconv, libdsp/blkconv.cxx:34-122): the upload of the spectrum tables,
// the data-movement variants, a bulk call, the host round trips, and the sfe_dsp_fir_* entry points.  What a handle works
// out before it uploads or launches -- tap partitions, the tables' arithmetic -- is fir_plan.h's; the checks of a call's
// buffers are call_checks.h's; the history epilogue and load_history are block.h's.  Host code only.
#include "host.h"

namespace sfe {

// ------------------------------------------------------------------------------ FIR

Fir *as_fir(void *h) { return as_handle<Fir>(h, "FIR"); }

// the tables of the 4096-point kernel (fir_plan.h) on the device
int FirTables::upload(const FirShape &sh, const float *taps)
{
    std::vector<v2f> w1, w2;
    fir_twiddles(w1, w2);
    int rc = hs.upload(fir_spectra<v2f>(sh, taps));
    if (rc == SFE_OK) rc = tw1.upload(w1);
    return rc != SFE_OK ? rc : tw2.upload(w2);
}

// A stream that is being captured into a hipGraph: the launches recorded now will be REPLAYED with the same
// arguments, so nothing of the stream's carried state may live on the host between a captured call and its
// replays.  A captured bulk call therefore (a) updates the history IN PLACE with the separate carry-over
// kernel behind the main launch (no double-buffer parity to flip on the host) and (b) is accepted only when
// its arguments do not depend on where in the stream it sits: n >= the history length, and for the
// resamplers an integer-valued step with n*U a multiple of it, so that every call starts in the time state
// the captured one started in.  Replaying the graph then processes the NEXT n samples found in d_in, exactly
// as the next eager call would (tests/test_gpu_graph.py).  VERDICT r2 item 8.
bool stream_is_capturing(hipStream_t s)
{
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cap) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return cap != hipStreamCaptureStatusNone;
}

// ---- which data-movement variant of the cf32 kernel (common.h: FIR_VAR_*) ------------------------
// The three variants compute the same bits and differ by a few percent in time, with a sign that
// depends on the box (profiles/r02/fir_walk_vs_tickets.txt against DESIGN.md 4.1's earlier tables:
// LDS-DMA from -5.7 % to +3.7 % against register loads).  Round 4: NOTHING IS
// MEASURED ON THE CALL PATH.  A stream call runs what sfe_dsp_fir_set_variant fixed, else what an
// earlier sfe_dsp_fir_calibrate call chose for this (device, channels, size class, overlap,
// per-channel taps), else register loads.  sfe_dsp_fir_calibrate is the measurement, made when the
// caller asks for it, synchronously and outside the stream: every variant over the caller's buffers
// (same output each time; the carried state and the stream position are not touched),
// FIR_CAL_ROUNDS interleaved rounds behind FIR_CAL_WARM_MS of launches, HIP events on the caller's
// stream; register loads unless another variant's median is more than 1 % ahead.
constexpr int FIR_CAL_ROUNDS = 9;                         // rounds that count: the LAST nine
constexpr float FIR_CAL_MARGIN = 0.99f;                   // another variant displaces register loads only by more than 1 %
constexpr int FIR_CAL_MAX_ROUNDS = 24;                    // ... of at most this many, and of at least FIR_CAL_WARM_MS of launches:
constexpr float FIR_CAL_WARM_MS = 80.0f;                  // the chip's first ~100 ms of work after idling run 5-6 % slow
struct FirVarKey {
    int device, n_channels, size_class, ovl, per_channel;
    bool operator<(const FirVarKey &o) const
    {
        return std::tie(device, n_channels, size_class, ovl, per_channel) < std::tie(o.device, o.n_channels, o.size_class, o.ovl, o.per_channel);
    }
};
static std::mutex g_fir_var_mutex;
static std::map<FirVarKey, int> g_fir_var_cache;

static FirVarKey fir_var_key(const Fir *f, const FirFftArgs &a)
{
    return FirVarKey{f->device, f->n_channels, fir_size_class(a.nblk, f->n_channels), f->ovl, f->per_channel};
}

static bool fir_has_variants(const Fir *f, const FirFftArgs &a)
{
    return f->parts == 1 && fir_fft_has_variants(a, f->data_complex, f->out_complex, f->in_u8, f->out_tx10, f->n_channels, 0);
}

// what a stream call runs: a map look-up, no device work
static int fir_pick_variant(Fir *f, const FirFftArgs &a)
{
    if (f->variant != FIR_VAR_AUTO) return f->variant;     // sfe_dsp_fir_set_variant
    if (!fir_has_variants(f, a)) return FIR_VAR_REG;
    std::lock_guard<std::mutex> lk(g_fir_var_mutex);
    auto it = g_fir_var_cache.find(fir_var_key(f, a));
    return it != g_fir_var_cache.end() ? it->second : FIR_VAR_REG;
}

// the measurement (sfe_dsp_fir_calibrate): `a` describes the call, a.hist_out == nullptr
static int fir_calibrate(Fir *f, FirFftArgs &a, hipStream_t s, int *chosen)
{
    *chosen = FIR_VAR_REG;
    if (!fir_has_variants(f, a)) return SFE_OK;             // one variant: nothing to choose
    Event e0, e1;
    int rc = e0.create(hipEventDefault);
    if (rc == SFE_OK) rc = e1.create(hipEventDefault);
    if (rc != SFE_OK) return rc;
    const int nvar = f->per_channel ? 2 : FIR_VAR_COUNT;      // per-channel taps: no wave-private instantiation
    float t[FIR_VAR_COUNT][FIR_CAL_ROUNDS];
    // interleaved rounds; a measurement made on a chip that has just come out of idle ranks the variants by
    // how they run at a clock the stream will never see again, so rounds go on until FIR_CAL_WARM_MS of
    // launches have run (and at least FIR_CAL_ROUNDS rounds) and only the last FIR_CAL_ROUNDS count
    float spent = 0.0f;
    for (int r = 0; r < FIR_CAL_MAX_ROUNDS && rc == SFE_OK && (r < FIR_CAL_ROUNDS || spent < FIR_CAL_WARM_MS); r++)
        for (int v = 0; v < nvar && rc == SFE_OK; v++) {
            a.variant = v;
            hipError_t e = hipEventRecord(e0, s);
            rc = launch_fir_fft(a, f->data_complex, f->out_complex, f->in_u8, f->out_tx10, f->n_channels, s, 0);
            if (rc != SFE_OK) break;
            if (e == hipSuccess) e = hipEventRecord(e1, s);
            if (e == hipSuccess) e = hipEventSynchronize(e1);
            float ms = 0.0f;
            if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
            if (e != hipSuccess) rc = hip_fail(e, "fir variant calibration");
            else {
                t[v][r % FIR_CAL_ROUNDS] = ms;         // a ring: the last FIR_CAL_ROUNDS rounds survive
                spent += ms;
            }
        }
    if (rc != SFE_OK) return rc;
    // Register loads are the reference point: with the straight-line store block they are the fastest or within
    // 0.5 % of it on every box of profiles/r03/fir_variants_box*.txt, where the three medians of one measurement lie
    // within 0.7 % of each other -- inside the noise of nine rounds.  Another variant is taken only when it is ahead
    // by more than 1 % (boxes on which LDS-DMA led by 4-6 % exist: DESIGN.md 4.1), the better of the two if both are.
    int best = FIR_VAR_REG;
    float best_ms = 0.0f;
    for (int v = 0; v < nvar; v++) {
        std::sort(t[v], t[v] + FIR_CAL_ROUNDS);
        const float med = t[v][FIR_CAL_ROUNDS / 2];
        f->cal_ms[v] = med;
        if (v == 0) best_ms = med * FIR_CAL_MARGIN;
        else if (med < best_ms) {
            best_ms = med;
            best = v;
        }
    }
    f->cal_runs++;
    {
        std::lock_guard<std::mutex> lk(g_fir_var_mutex);
        g_fir_var_cache[fir_var_key(f, a)] = best;
    }
    *chosen = best;
    return SFE_OK;
}

// the launch description of one bulk call over the transform kernel (partition 0)
static void fir_fill_args(const Fir *f, FirFftArgs &a, const void *d_in, void *d_out, size_t n, size_t in_stride,
                          size_t out_stride)
{
    a.in = d_in;
    a.out = d_out;
    a.hist = f->hist.cur();
    a.tw1 = f->tab.tw1;
    a.tw2 = f->tab.tw2;
    a.n = (long long)n;
    a.in_stride = (long long)in_stride;
    a.out_stride = (long long)out_stride;
    a.hl = f->ovl;
    a.advance = FFT_N - f->ovl;
    a.hist_len = f->hl;
    a.nblk = ((long long)n + a.advance - 1) / a.advance;
    a.ticket = f->ticket;
    a.total = 0;
    a.tgroups = 0;
    a.hs_stride = f->per_channel ? (long long)f->parts * 16 * 256 : 0;
    a.variant = FIR_VAR_AUTO;
    a.hs = f->tab.hs;
    a.shift = 0;
    a.hist_out = nullptr;
}

int fir_run(Fir *f, const void *d_in, void *d_out, size_t n, size_t in_stride,
                   size_t out_stride, hipStream_t s)
{
    if (n == 0) return SFE_OK;
    f->started = true;
    int algo = f->algo;
    if (algo == SFE_FIR_ALGO_AUTO) algo = f->fft_ok ? SFE_FIR_ALGO_FFT : SFE_FIR_ALGO_DIRECT;
    int rc;
    bool hist_fused = false;
    const bool capturing = stream_is_capturing(s);
    if (capturing && n < (size_t)f->hl) {
        set_error("fir_process_stream: a call captured into a hipGraph must bring at least the history length (%d samples): "
                  "shorter calls carry state the replay cannot see", f->hl);
        return SFE_ESTATE;
    }
    if (algo == SFE_FIR_ALGO_FFT) {
        if (!f->fft_ok) {
            set_error("fir: %d taps exceed %d partitions of the 4096-point kernel", f->n_taps, FIR_MAX_PARTS);
            return SFE_EINVAL;
        }
        FirFftArgs a;
        fir_fill_args(f, a, d_in, d_out, n, in_stride, out_stride);
        hist_fused = n >= (size_t)f->hl && !capturing;   // else the old history still contributes (captured: in place, below)
        a.variant = fir_pick_variant(f, a);
        f->last_variant = a.variant;
        rc = SFE_OK;
        // one launch per tap partition: partition p filters the stream delayed by p*ovl samples and
        // (p > 0) adds to what the earlier ones wrote
        for (int p = 0; p < f->parts && rc == SFE_OK; p++) {
            a.hs = f->tab.hs.p + (size_t)p * 16 * 256;
            a.shift = p * f->ovl;
            a.hist_out = (p == 0 && hist_fused) ? f->hist.next() : nullptr;
            rc = launch_fir_fft(a, f->data_complex, f->out_complex, f->in_u8, f->out_tx10, f->n_channels, s, p > 0);
        }
    } else {
        if (f->taps_complex || f->in_u8 || f->out_tx10 || f->per_channel) {
            set_error("fir: the direct kernel takes one set of real taps and float input/output; use SFE_FIR_ALGO_FFT");
            return SFE_EINVAL;
        }
        const PolyTiledPlan *pl = get_tiled_plan(f->plans, f->h_taps, 1, f->n_taps, 1, 0, &rc);
        if (rc != SFE_OK) return rc;
        const PolyIo io{d_in, d_out, (long long)n, (long long)in_stride, (long long)out_stride};
        if (pl) {
            PolyTiledArgs ta;
            fill_io(ta, f, io);
            ta.G = pl->d_G;
            ta.Gt = pl->d_Gt;
            ta.n_out = (long long)n;
            ta.Lp = pl->Lp;
            ta.e_max = pl->e_max;
            rc = launch_poly_tiled(*pl, ta, f->data_complex, 0, 0, f->n_channels, s);
        } else {
            PolyArgs a;
            memset(&a, 0, sizeof(a));
            fill_io(a, f, io);
            a.taps = f->d_taps;
            a.U = 1;
            a.plen = f->n_taps;
            a.step = 1;
            a.n_out = (long long)n;
            rc = launch_poly_int(a, f->data_complex, 0, 0, f->n_channels, s);
        }
    }
    if (rc != SFE_OK) return rc;
    return carry_history(f->hist, f->captured, d_in, n, in_stride, f->hl, f->data_complex ? 2 : 1, f->n_channels, f->in_u8, hist_fused, capturing, s);
}

// the checks of a bulk call's buffers (call_checks.h: channels), behind the entry point's null rule: sfe_dsp_fir_process_stream
// and, over the same buffers, sfe_dsp_fir_calibrate
static int fir_check_buffers(const char *who, const Fir *f, const void *d_in, const void *d_out, size_t n, size_t in_stride, size_t out_stride)
{
    static const ChannelNouns nouns{"channel stride smaller than n", "cf32 8 B, f32 4 B, u8 (I,Q) pairs 2 B; 10-bit output: none", true};
    // bytes per element as the kernels address them
    const size_t isz = f->in_u8 ? (f->data_complex ? 2 : 1) : (f->data_complex ? 8 : 4);
    return check_channels(who, nouns, (size_t)f->n_channels, d_in, n, in_stride, isz, d_out, n, out_stride, f->out_complex ? 8 : 4, f->out_tx10 != 0);
}

// One host round trip on the handle's own stream: m samples that sit in the pinned buffer `h`, and the wait for their
// outputs.  Zero-copy (m <= zc_max, where the kernel reads its input once: parts == 1): the kernel reads `h` and writes the
// pinned `h_zc` itself -- one launch and one wait; else staged: copy in, launch, copy back into `h`, wait.  *res: where
// the outputs are.
static int fir_round_trip(Fir *f, size_t m, void *h, void *h_zc, void *d_in, void *d_out, const void **res)
{
    const bool zc = f->parts == 1 && h_zc && m <= f->zc_max;
    if (!zc) SFE_HIP(hipMemcpyAsync(d_in, h, m * (f->data_complex ? 8 : 4), hipMemcpyHostToDevice, f->stream));
    const int rc = fir_run(f, zc ? h : d_in, zc ? h_zc : d_out, m, m, m, f->stream);
    if (rc != SFE_OK) return rc;
    if (!zc) SFE_HIP(hipMemcpyAsync(h, d_out, m * (f->out_complex ? 8 : 4), hipMemcpyDeviceToHost, f->stream));
    SFE_HIP(hipStreamSynchronize(f->stream));
    *res = zc ? h_zc : h;
    return SFE_OK;
}

// the spectra a handle's taps give for `parts` partitions at overlap `ovl`
static FirShape fir_shape(const Fir *f, int parts, int ovl)
{
    return FirShape{f->n_taps, f->taps_complex, f->per_channel ? f->n_channels : 1, parts, ovl};
}

static int fir_create_impl(const float *taps, int n_taps, int taps_complex, int data_complex,
                           int n_channels, int block_hint, int device, int per_channel, sfe_fir_t *out)
{
    if (!out) return SFE_EINVAL;
    *out = nullptr;
    if (!taps || n_taps < 1 || n_channels < 1) {
        set_error("fir_create: need taps, n_taps >= 1, n_channels >= 1");
        return SFE_EINVAL;
    }
    if (block_hint != 0 && block_hint + 1 - n_taps < 1) {
        set_error("fir_create: fft_len %d leaves no block for %d taps (blkconv.cxx:47)", block_hint, n_taps);
        return SFE_EINVAL;
    }
    CreateScope scope(device);
    if (scope.rc != SFE_OK) return scope.rc;
    std::unique_ptr<Fir> f(new (std::nothrow) Fir);
    if (!f) return SFE_ENOMEM;
    f->n_taps = n_taps;
    f->taps_complex = taps_complex ? 1 : 0;
    f->data_complex = data_complex ? 1 : 0;
    f->out_complex = (f->taps_complex || f->data_complex) ? 1 : 0;
    f->n_channels = n_channels;
    f->per_channel = per_channel ? 1 : 0;
    f->device = device;
    f->block_hint = block_hint;
    f->blk = block_hint ? block_hint + 1 - n_taps : 0;
    f->fft_ok = fir_choose_partition(n_taps, &f->ovl, &f->parts);
    if (f->per_channel && !f->fft_ok) {
        set_error("fir_create_per_channel: %d taps exceed %d partitions of the 4096-point kernel", n_taps, FIR_MAX_PARTS);
        return SFE_ERANGE;
    }
    f->hl = fir_history_len(n_taps);
    int rc = f->stream.create();
    if (rc != SFE_OK) return rc;
    f->h_taps_all.assign(taps, taps + (size_t)n_taps * (taps_complex ? 2 : 1) * (per_channel ? n_channels : 1));
    if (f->fft_ok && ((rc = f->tab.upload(fir_shape(f.get(), f->parts, f->ovl), taps)) != SFE_OK ||
                      (rc = f->ticket.alloc_zero(FIR_TICKET_GROUPS_MAX * 128 / sizeof(unsigned))) != SFE_OK))
        return rc;
    if (!f->taps_complex && !f->per_channel) {
        f->h_taps.assign(taps, taps + n_taps);
        if ((rc = f->d_taps.upload(f->h_taps)) != SFE_OK) return rc;
    }
    if ((rc = f->hist.alloc_zero(f->hist_bytes())) != SFE_OK) return rc;
    if (f->blk > 0) {
        if (n_channels != 1) {
            set_error("fir_create: the host block path (block_hint) is single-channel");
            return SFE_EINVAL;
        }
        const size_t in_e = f->data_complex ? 2 : 1, out_e = f->out_complex ? 2 : 1;
        const size_t hf = ((size_t)block_hint + 2) * (out_e > in_e ? out_e : in_e);       // floats of a pinned block
        if ((rc = f->h_buf.alloc(hf)) != SFE_OK) return rc;
        memset(f->h_buf, 0, hf * sizeof(float));
        if ((rc = f->d_blk_in.alloc((size_t)f->blk * in_e * sizeof(float))) != SFE_OK ||
            (rc = f->d_blk_out.alloc((size_t)f->blk * out_e * sizeof(float))) != SFE_OK || (rc = f->h_blk_out.alloc(hf * sizeof(float))) != SFE_OK)
            return rc;
    }
    SFE_HIP(hipDeviceSynchronize());
    *out = f.release();
    return SFE_OK;
}

}  // namespace sfe

using namespace sfe;

extern "C" {

// ---------------------------------------------------------------------------- FIR
int sfe_dsp_fir_create(const float *taps, int n_taps, int taps_complex, int data_complex,
                       int n_channels, int block_hint, int device, sfe_fir_t *out)
{
    return fir_create_impl(taps, n_taps, taps_complex, data_complex, n_channels, block_hint, device, 0, out);
}

int sfe_dsp_fir_create_per_channel(const float *taps, int n_taps, int taps_complex, int n_channels, int device,
                                   sfe_fir_t *out)
{
    return fir_create_impl(taps, n_taps, taps_complex, 1, n_channels, 0, device, 1, out);
}

int sfe_dsp_fir_plan(int n_taps, int *overlap, int *partitions, int *advance)
{
    if (n_taps < 1) return SFE_EINVAL;
    int o = 0, p = 0;
    if (!fir_choose_partition(n_taps, &o, &p)) {
        set_error("fir_plan: %d taps exceed %d partitions of the 4096-point kernel", n_taps, FIR_MAX_PARTS);
        return SFE_ERANGE;
    }
    if (overlap) *overlap = o;
    if (partitions) *partitions = p;
    if (advance) *advance = FFT_N - o;
    return SFE_OK;
}

int sfe_dsp_fir_host_buffer(sfe_fir_t h, float **buf, int *blk)
{
    Fir *f = as_fir(h);
    if (!f || !f->h_buf) {
        set_error("fir_host_buffer: handle was created without block_hint");
        return SFE_ESTATE;
    }
    if (buf) *buf = f->h_buf;
    if (blk) *blk = f->blk;
    return SFE_OK;
}

int sfe_dsp_fir_process_block(sfe_fir_t h)
{
    Fir *f = as_fir(h);
    if (!f || !f->h_buf) {
        set_error("fir_process_block: handle was created without block_hint");
        return SFE_ESTATE;
    }
    SFE_ON_DEVICE(f->device);
    const void *res = nullptr;
    const int rc = fir_round_trip(f, (size_t)f->blk, f->h_buf, f->h_blk_out, f->d_blk_in, f->d_blk_out, &res);
    if (rc == SFE_OK && res != f->h_buf) memcpy(f->h_buf, res, (size_t)f->blk * (f->out_complex ? 8 : 4));
    return rc;
}

int sfe_dsp_fir_process_stream(sfe_fir_t h, const void *d_in, void *d_out, size_t n,
                               size_t in_stride, size_t out_stride, sfe_stream_t stream)
{
    Fir *f = as_fir(h);
    if (!f || (n && (!d_in || !d_out))) {
        set_error("fir_process_stream: null handle or buffer");
        return SFE_EINVAL;
    }
    const int rc = fir_check_buffers("fir_process_stream", f, d_in, d_out, n, in_stride, out_stride);
    if (rc != SFE_OK) return rc;
    SFE_ON_DEVICE(f->device);
    return fir_run(f, d_in, d_out, n, in_stride, out_stride, (hipStream_t)stream);
}

int sfe_dsp_fir_process_host(sfe_fir_t h, const void *in, void *out, size_t n)
{
    Fir *f = as_fir(h);
    if (!f || (n && (!in || !out))) {
        set_error("fir_process_host: null handle or buffer");
        return SFE_EINVAL;
    }
    if (f->n_channels != 1) {
        set_error("fir_process_host: single-channel handles only");
        return SFE_EINVAL;
    }
    SFE_ON_DEVICE(f->device);
    const size_t in_e = f->data_complex ? 8 : 4, out_e = f->out_complex ? 8 : 4;
    const size_t CH = (size_t)1 << 20;            // samples per staged chunk
    if (!f->stage.h) {
        // build the set beside the handle and move it in only when all of it exists: a failed later allocation must
        // not leave a half-built staging set behind for the next call to trip over
        FirStage st;
        const size_t zc = f->zc_max < CH ? f->zc_max : CH;
        int rc = st.h.alloc(CH * (in_e > out_e ? in_e : out_e));
        if (rc == SFE_OK) rc = st.d_in.alloc(CH * in_e);
        if (rc == SFE_OK) rc = st.d_out.alloc(CH * out_e);
        if (rc == SFE_OK && zc) rc = st.h_out.alloc(zc * out_e);
        if (rc != SFE_OK) return rc;
        f->stage = std::move(st);
    }
    const char *ip = static_cast<const char *>(in);
    char *op = static_cast<char *>(out);
    for (size_t off = 0; off < n; off += CH) {
        const size_t m = n - off < CH ? n - off : CH;
        memcpy(f->stage.h, ip + off * in_e, m * in_e);
        const void *res = nullptr;
        const int rc = fir_round_trip(f, m, f->stage.h, f->stage.h_out, f->stage.d_in, f->stage.d_out, &res);
        if (rc != SFE_OK) return rc;
        memcpy(op + off * out_e, res, m * out_e);
    }
    return SFE_OK;
}

// carried state from a halo (block.h: load_history)
int sfe_dsp_fir_load_history(sfe_fir_t h, const void *d_prev, size_t n_prev, size_t stride, sfe_stream_t stream)
{
    return load_history("fir_load_history", as_fir(h), d_prev, n_prev, stride, (hipStream_t)stream);
}

int sfe_dsp_fir_set_input_format(sfe_fir_t h, int fmt)
{
    Fir *f = as_fir(h);
    if (!f || (fmt != SFE_FMT_F32 && fmt != SFE_FMT_U8)) return SFE_EINVAL;
    if (f->piped && (fmt == SFE_FMT_U8) != (f->in_u8 != 0)) {
        // a pipe sized its pinned and device batches from the item format at create
        set_error("fir_set_input_format: a pipe over this handle has frozen its item format (destroy the pipe first)");
        return SFE_ESTATE;
    }
    if (fmt == SFE_FMT_U8 && (!f->fft_ok || f->taps_complex)) {
        set_error("fir_set_input_format: u8 input needs the FFT kernel with real taps");
        return SFE_ESTATE;
    }
    f->in_u8 = fmt == SFE_FMT_U8;
    return SFE_OK;
}

// A filter of ~2818..3841 taps is served fastest by TWO partitions (fir_choose_partition), but the
// 10-bit packed output exists for the single-launch kernel only (partitions after the first
// read-modify-write float32).  One transform can still overlap such a filter (hl1 < 4096), so the
// handle is re-planned as ONE partition: new spectrum table, new (zeroed) history.  ADVICE r2.
static int fir_replan_single(Fir *f)
{
    const int hl1 = fir_single_overlap(f->n_taps);
    if (hl1 >= FFT_N) return SFE_ESTATE;
    if (f->started || f->captured) {
        // the re-plan zeroes the carried state and frees buffers a captured graph names
        set_error("fir_set_output_format: this filter must be re-planned as one launch for 10-bit output, which "
                  "restarts the stream: set the format before the first process call (or after sfe_dsp_fir_reset)");
        return SFE_ESTATE;
    }
    SFE_HIP(hipDeviceSynchronize());
    // build the new plan beside the old one and move it in only when all of it exists: a failure leaves the handle as it was
    FirTables tab;
    CarriedPair hist;
    int rc = tab.upload(fir_shape(f, 1, hl1), f->h_taps_all.data());        // (the work counters are the handle's and stay: zero between launches)
    if (rc == SFE_OK) rc = hist.alloc_zero((size_t)f->n_channels * hl1 * (f->data_complex ? 8 : 4));
    if (rc != SFE_OK) return rc;
    f->tab = std::move(tab);        // (the old tables and history go with the locals)
    f->hist = std::move(hist);
    f->parts = 1;
    f->ovl = f->hl = hl1;
    return SFE_OK;
}

int sfe_dsp_fir_set_output_format(sfe_fir_t h, int fmt)
{
    Fir *f = as_fir(h);
    if (!f || (fmt != SFE_FMT_F32 && fmt != SFE_FMT_TX10)) return SFE_EINVAL;
    if (f->piped && (fmt == SFE_FMT_TX10) != (f->out_tx10 != 0)) {
        set_error("fir_set_output_format: a pipe over this handle has frozen its item format (destroy the pipe first)");
        return SFE_ESTATE;
    }
    if (fmt == SFE_FMT_TX10 && f->fft_ok && f->parts > 1 && f->data_complex == f->out_complex) {
        // up to 3841 taps one transform still overlaps the filter: re-plan as a single launch (the carried state is zeroed:
        // formats are set before a stream starts)
        SFE_ON_DEVICE(f->device);
        int rc = fir_replan_single(f);
        if (rc != SFE_OK && rc != SFE_ESTATE) return rc;
    }
    if (fmt == SFE_FMT_TX10 && (!f->fft_ok || f->parts > 1 || f->data_complex != f->out_complex)) {
        set_error("fir_set_output_format: 10-bit output needs the single-launch FFT kernel (a filter that one 4096-point "
                  "transform can overlap: up to 3841 taps) and a real->real or complex->complex stream");
        return SFE_ESTATE;
    }
    f->out_tx10 = fmt == SFE_FMT_TX10;
    return SFE_OK;
}

int sfe_dsp_fir_set_algo(sfe_fir_t h, int algo)
{
    Fir *f = as_fir(h);
    if (!f || algo < SFE_FIR_ALGO_AUTO || algo > SFE_FIR_ALGO_FFT) return SFE_EINVAL;
    f->algo = algo;
    return SFE_OK;
}

int sfe_dsp_fir_set_variant(sfe_fir_t h, int variant)
{
    Fir *f = as_fir(h);
    if (!f || variant < SFE_FIR_VARIANT_AUTO || variant > SFE_FIR_VARIANT_WAVE_PRIVATE) {
        set_error("fir_set_variant: -1 (measure) or 0..2");
        return SFE_EINVAL;
    }
    f->variant = variant;
    return SFE_OK;
}

int sfe_dsp_fir_get_variant(sfe_fir_t h, int *last_variant, int *calibrations, float *ms_by_variant)
{
    Fir *f = as_fir(h);
    if (!f) return SFE_EINVAL;
    if (last_variant) *last_variant = f->last_variant;
    if (calibrations) *calibrations = f->cal_runs;
    if (ms_by_variant)
        for (int v = 0; v < FIR_VAR_COUNT; v++) ms_by_variant[v] = f->cal_ms[v];
    return SFE_OK;
}

int sfe_dsp_fir_calibrate(sfe_fir_t h, const void *d_in, void *d_out, size_t n, size_t in_stride,
                          size_t out_stride, sfe_stream_t stream, int *chosen)
{
    Fir *f = as_fir(h);
    if (chosen) *chosen = SFE_FIR_VARIANT_REGISTER_LOADS;
    if (!f || !n || !d_in || !d_out) {
        set_error("fir_calibrate: null handle or buffer");
        return SFE_EINVAL;
    }
    int rc = fir_check_buffers("fir_calibrate", f, d_in, d_out, n, in_stride, out_stride);      // it launches over them
    if (rc != SFE_OK) return rc;
    if (!f->fft_ok || f->algo == SFE_FIR_ALGO_DIRECT) return SFE_OK;    // the direct kernel has one form
    SFE_ON_DEVICE(f->device);
    hipStream_t s = (hipStream_t)stream;
    if (stream_is_capturing(s)) {
        set_error("fir_calibrate: a measurement cannot be captured into a hipGraph");
        return SFE_ESTATE;
    }
    FirFftArgs a;
    fir_fill_args(f, a, d_in, d_out, n, in_stride, out_stride);      // hist_out stays null: the stream does not advance
    int best = FIR_VAR_REG;
    rc = fir_calibrate(f, a, s, &best);
    if (rc == SFE_OK && chosen) *chosen = best;
    return rc;
}

int sfe_dsp_fir_forget_calibrations(void)
{
    std::lock_guard<std::mutex> lk(g_fir_var_mutex);
    g_fir_var_cache.clear();
    return SFE_OK;
}

int sfe_dsp_fir_set_zero_copy_max(sfe_fir_t h, size_t max_samples)
{
    Fir *f = as_fir(h);
    if (!f) return SFE_EINVAL;
    if (f->stage.h) {
        // the pinned output staging of sfe_dsp_fir_process_host was sized from the old limit
        set_error("fir_set_zero_copy_max: set it before the first sfe_dsp_fir_process_host call");
        return SFE_ESTATE;
    }
    f->zc_max = max_samples;
    return SFE_OK;
}

int sfe_dsp_fir_reset(sfe_fir_t h)
{
    Fir *f = as_fir(h);
    if (!f) return SFE_EINVAL;
    SFE_ON_DEVICE(f->device);
    SFE_HIP(hipDeviceSynchronize());
    const int rc = f->hist.zero();
    if (rc != SFE_OK) return rc;
    if (f->ticket) SFE_HIP(hipMemset(f->ticket, 0, FIR_TICKET_GROUPS_MAX * 128));
    f->started = false;         // `captured` stays: a graph made before the reset still names hist.cur()
    return SFE_OK;
}

int sfe_dsp_fir_destroy(sfe_fir_t h)
{
    Fir *f = as_fir(h);
    if (!f) return SFE_OK;
    if (f->piped) {
        set_error("fir_destroy: a pipe still borrows this handle (sfe_dsp_pipe_destroy first)");
        return SFE_ESTATE;
    }
    return destroy_handle(f);
}

}  // extern "C"
