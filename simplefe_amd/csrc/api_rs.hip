// api_rs.hip -- the resample / decimate handle behind sfe_rs_t (libdsp/resample.cxx:37-153, libdsp/decimate.cxx:37-140):
// a call's checks, the choice of kernel, the upload of the plans, carried state, and the sfe_dsp_rs_* entry points.  What a call
// works out before it launches -- the integer-step closed form, the general-rate plan and its run memo -- is rs_plan.h's.
// Host code only.
#include "host.h"
#include <stdlib.h>

namespace sfe {

// ------------------------------------------------------------------ resample / decimate

Rs *as_rs(void *h) { return as_handle<Rs>(h, "resample/decimate"); }

// the class-compatible path's buffers double from 1024; its staging is sized exactly
static size_t rs_doubled(size_t cap, size_t n)
{
    if (!cap) cap = 1024;
    while (cap < n) cap *= 2;
    return cap;
}
static int rs_ensure_sched(Rs *r, size_t n) { return r->sched.reserve(n, rs_doubled(r->sched.cap, n)); }
static int rs_ensure_out(Rs *r, size_t n)
{
    const size_t e = (size_t)r->esz();
    return r->d_out.reserve(n * e, rs_doubled(r->d_out.cap / e, n) * e);
}

// the generic kernels' arguments (launch_poly_int, launch_poly_sched): the caller adds the law -- pos0 / step or the schedule
static PolyArgs rs_poly_args(const Rs *r, const PolyIo &io)
{
    PolyArgs a;
    memset(&a, 0, sizeof(a));
    fill_io(a, r, io);
    a.taps = r->d_taps;
    a.U = r->U;
    a.plen = r->plen;
    return a;
}

}  // namespace sfe

using namespace sfe;

extern "C" {

// ------------------------------------------------------------------ resample / decimate
int sfe_dsp_rs_plan(sfe_rs_timestate *state, int upsample, int n_in, int out_len, float rate,
                    int32_t *rel_pos, float *mu, int cap, int *n_out)
{
    if (!state || upsample < 1 || n_in < 0 || !n_out) return SFE_EINVAL;
    int overflow = 0, k = 0;
    const int n = time_law(state, upsample, n_in, out_len, rate, [&](int p, float m) {
        if (k < cap) {
            if (rel_pos) rel_pos[k] = p;
            if (mu) mu[k] = m;
        } else overflow = 1;
        k++;
    });
    *n_out = n;
    return overflow ? SFE_ERANGE : SFE_OK;
}

int sfe_dsp_rs_create(const float *taps, int n_taps, int upsample, int blksize, int data_complex,
                      int n_channels, int device, int mode, sfe_rs_t *out)
{
    if (!out) return SFE_EINVAL;
    *out = nullptr;
    if (!taps || n_taps < 1 || upsample < 1 || blksize < 1 || n_channels < 1 ||
        (mode != SFE_RS_RESAMPLE && mode != SFE_RS_DECIMATE)) {
        set_error("rs_create: bad arguments");
        return SFE_EINVAL;
    }
    CreateScope scope(device);
    if (scope.rc != SFE_OK) return scope.rc;
    std::unique_ptr<Rs> r(new (std::nothrow) Rs);
    if (!r) return SFE_ENOMEM;
    r->U = upsample;
    r->n_taps = n_taps;
    r->blksize = blksize;
    r->data_complex = data_complex ? 1 : 0;
    r->n_channels = n_channels;
    r->device = device;
    r->mode = mode;
    // decimate appends a zero tap when n_taps is even (decimate.cxx:42-51); resample pads the
    // last phase with zeros (resample.cxx:43,55-64).  Both are "ceil to a whole phase row".
    const int eff = (mode == SFE_RS_DECIMATE && (n_taps % 2 == 0)) ? n_taps + 1 : n_taps;
    r->plen = (eff + upsample - 1) / upsample;
    r->hl = ((r->plen + 1 + 63) / 64) * 64;
    int rc = r->stream.create();
    if (rc != SFE_OK) return rc;
    std::vector<float> &pm = r->h_taps_pm;
    pm.assign((size_t)upsample * r->plen, 0.0f);
    for (int j = 0; j < upsample; j++)
        for (int i = 0; i < r->plen; i++) {
            const int n = i * upsample + j;
            pm[(size_t)j * r->plen + i] = n < n_taps ? taps[n] : 0.0f;
        }
    if ((rc = r->d_taps.upload(pm)) != SFE_OK || (rc = r->hist.alloc_zero((size_t)n_channels * r->hl * r->esz())) != SFE_OK ||
        (rc = r->d_in.alloc((size_t)blksize * r->esz())) != SFE_OK ||
        (rc = r->d_ticket.alloc_zero(POLY_TICKET_GROUPS * 128 / sizeof(unsigned))) != SFE_OK)
        return rc;
    SFE_HIP(hipDeviceSynchronize());
    *out = r.release();
    return SFE_OK;
}

int sfe_dsp_rs_process(sfe_rs_t h, const float *in, int n_in, float *out, int out_len, float rate,
                       int *n_out)
{
    Rs *r = as_rs(h);
    if (!r || !n_out) return SFE_EINVAL;
    *n_out = 0;
    if (r->n_channels != 1) {
        set_error("rs_process: the host-pointer call is single-channel");
        return SFE_EINVAL;
    }
    // parameter checks, messages and "return 0 outputs" as the reference
    if (r->mode == SFE_RS_RESAMPLE) {
        if (n_in > r->blksize || rate < 1.0 / r->U) {                      // resample.cxx:91-94
            printf("input parameter is wrong, rate <= 1/upsample, n_in <= blksize\n");
            return SFE_OK;
        }
    } else {
        if (rate < 1.0) {                                                  // decimate.cxx:75-78
            printf("rate should be larger than 1.0\n");
            return SFE_OK;
        }
        if (n_in > r->blksize) {                                           // decimate.cxx:79-82
            printf("number of samples should be less than blksize\n");
            return SFE_OK;
        }
    }
    if (out_len < floorf(n_in * 1.0f / rate)) {                            // resample.cxx:95-98
        printf("output buffer is not large enough");
        return SFE_OK;
    }
    if (n_in < 0 || out_len < 0 || (n_in && !in) || (out_len && !out)) return SFE_EINVAL;
    SFE_ON_DEVICE(r->device);

    // The common call -- out_len roomy enough that the law, not the buffer, ends the outputs -- is the
    // bulk path on one block with the reference's arithmetic order (exact): the tiled / run-length kernels
    // stage the block in LDS instead of two global dot products per output, the outputs are written
    // straight into pinned host memory, and the stream sees copy-in, kernel, history instead of seven
    // operations.  Same bits (tests/test_gpu_parity.py: class calls against the compiled reference).
    if (n_in > 0 && !r->in_u8) {
        const float stepf = rate * (float)r->U;
        bool roomy;
        if (rs_int_step_law(stepf, r->ts, r->blksize, r->U))
            roomy = rs_int_call(r->ts, r->U, n_in, (long long)stepf).K <= (long long)out_len;
        else
            roomy = (long long)out_len >= (long long)ceilf((float)n_in / rate) + 2;
        if (roomy) {
            const size_t in_b = (size_t)n_in * r->esz(), out_off = (in_b + 255) & ~(size_t)255;
            int rc = r->h_stage.reserve(out_off + ((size_t)out_len + 1) * r->esz());
            if (rc != SFE_OK) return rc;
            char *h_out = r->h_stage->p + out_off;
            memcpy(r->h_stage->p, in, in_b);
            SFE_HIP(hipMemcpyAsync(r->d_in, r->h_stage->p, in_b, hipMemcpyHostToDevice, r->stream));
            const int keep = r->exact_stream;
            r->exact_stream = 1;
            size_t n = 0;
            rc = sfe_dsp_rs_process_stream(h, r->d_in, (size_t)n_in, (size_t)n_in, h_out, (size_t)out_len, (size_t)out_len,
                                           rate, &n, r->stream);
            r->exact_stream = keep;
            if (rc != SFE_OK) return rc;
            SFE_HIP(hipStreamSynchronize(r->stream));
            if (n) memcpy(out, h_out, n * r->esz());
            *n_out = (int)n;
            return SFE_OK;
        }
    }

    int rc = rs_ensure_sched(r, (size_t)out_len + 1);
    if (rc != SFE_OK) return rc;
    rc = rs_ensure_out(r, (size_t)out_len + 1);
    if (rc != SFE_OK) return rc;
    const size_t in_b = (size_t)n_in * r->esz();
    const size_t out_b = ((size_t)out_len + 1) * r->esz();
    rc = r->h_stage.reserve(in_b > out_b ? in_b : out_b);
    if (rc != SFE_OK) return rc;
    Rs::Sched &sc = r->sched.b;

    int k = 0;
    const int n = time_law(&r->ts, r->U, n_in, out_len, rate, [&](int p, float m) {
        sc.pos.h.p[k] = p;
        sc.mu.h.p[k] = m;
        k++;
    });
    if (n_in) {
        memcpy(r->h_stage->p, in, in_b);
        SFE_HIP(hipMemcpyAsync(r->d_in, r->h_stage->p, in_b, hipMemcpyHostToDevice, r->stream));
    }
    if (n > 0) {
        SFE_HIP(hipMemcpyAsync(sc.pos.d, sc.pos.h, (size_t)n * sizeof(long long), hipMemcpyHostToDevice, r->stream));
        SFE_HIP(hipMemcpyAsync(sc.mu.d, sc.mu.h, (size_t)n * sizeof(float), hipMemcpyHostToDevice, r->stream));
        PolyArgs a = rs_poly_args(r, PolyIo{r->d_in, r->d_out->p, n_in, n_in, n});
        a.n_out = n;
        a.sched_pos = sc.pos.d;
        a.sched_mu = sc.mu.d;
        rc = launch_poly_sched(a, r->data_complex, 1, 1, r->stream);
        if (rc != SFE_OK) return rc;
    }
    rc = carry_history(r->hist, r->captured, r->d_in, (size_t)n_in, (size_t)n_in, r->hl, r->data_complex ? 2 : 1, 1, 0, false, false, r->stream);
    if (rc != SFE_OK) return rc;
    if (n > 0) SFE_HIP(hipMemcpyAsync(r->h_stage->p, r->d_out->p, (size_t)n * r->esz(), hipMemcpyDeviceToHost, r->stream));
    SFE_HIP(hipStreamSynchronize(r->stream));
    if (n > 0) memcpy(out, r->h_stage->p, (size_t)n * r->esz());
    *n_out = n;
    return SFE_OK;
}

static int rs_process_stream_impl(sfe_rs_t h, const void *d_in, size_t n_in, size_t in_stride,
                                  void *d_out, size_t out_cap, size_t out_stride, float rate,
                                  size_t *n_out, sfe_stream_t stream);

int sfe_dsp_rs_process_stream(sfe_rs_t h, const void *d_in, size_t n_in, size_t in_stride,
                              void *d_out, size_t out_cap, size_t out_stride, float rate,
                              size_t *n_out, sfe_stream_t stream)
{
    Rs *r = as_rs(h);
    if (r) r->u8_refused = false;
    int rc = rs_process_stream_impl(h, d_in, n_in, in_stride, d_out, out_cap, out_stride, rate, n_out, stream);
    if (rc != SFE_ESTATE || !r || !r->in_u8 || !r->u8_refused) return rc;
    // Wire-format input on a shape that has no fused u8 kernel (integer steps beyond the tiled kernels' -- more than 64 samples or 8 outputs per
    // period --, a general rate the transform-domain kernel does not take): until round 5 such a call was REFUSED.  Nothing has been launched and
    // no state touched: convert the call's bytes once (the same (b - 128) * (1 / 127) as every fused path: the same bits) and run the float path.
    SFE_ON_DEVICE(r->device);
    hipStream_t s = (hipStream_t)stream;
    const size_t w = r->data_complex ? 2 : 1, floats = (size_t)r->n_channels * n_in * w;
    if (floats > r->d_u8f.cap) {
        if (stream_is_capturing(s)) {
            set_error("rs_process_stream: this u8 call needs %zu bytes of conversion scratch, which cannot be allocated while the stream is being captured",
                      floats * 4);
            return SFE_ESTATE;
        }
        if ((rc = r->d_u8f.reserve(floats)) != SFE_OK) return rc;
    } else if (r->u8f_stream != s && r->u8f_stream) {
        SFE_HIP(hipStreamSynchronize(r->u8f_stream));         // the previous call on another stream may still read the scratch
    }
    r->u8f_stream = s;
    for (int c = 0; c < r->n_channels; c++) {
        rc = launch_rx_u8_to_f32(static_cast<const uint8_t *>(d_in) + (size_t)c * in_stride * w, r->d_u8f->p + (size_t)c * n_in * w, n_in * w, s);
        if (rc != SFE_OK) return rc;
    }
    r->in_u8 = 0;
    rc = rs_process_stream_impl(h, r->d_u8f->p, n_in, n_in, d_out, out_cap, out_stride, rate, n_out, stream);
    r->in_u8 = 1;
    return rc;
}

}  // extern "C"

// ------------------------------------------------------------------ one process_stream call, step by step
namespace {

struct RsCall {                 // the call's arguments, past its checks
    PolyIo io;
    size_t n_in, out_cap;
    float rate, stepf;          // stepf = fl(rate * U)
    hipStream_t s;
    bool capturing;
};

// The checks in front of the device: SFE_OK with n_in == 0 is a call with nothing to do (the caller returns as well).
int rs_check_call(const Rs *r, const void *d_in, size_t n_in, size_t in_stride, void *d_out, size_t out_cap, size_t out_stride, float rate)
{
    if (r->mode == SFE_RS_RESAMPLE ? (rate < 1.0 / r->U) : (rate < 1.0)) {
        set_error("rs_process_stream: rate %g not accepted by this mode", (double)rate);
        return SFE_EINVAL;
    }
    if (n_in == 0) return SFE_OK;
    if (!d_in || !d_out) {
        set_error("rs_process_stream: null buffer");
        return SFE_EINVAL;
    }
    // out_cap outputs per channel may be written: a smaller stride would let channels overwrite each other
    static const ChannelNouns nouns{"channel stride smaller than the channel (in_stride >= n_in, out_stride >= out_cap)",
                                    "cf32 8 B, f32 4 B, u8 (I,Q) pairs 2 B", false};
    const size_t isz = r->in_u8 ? (r->data_complex ? 2 : 1) : (size_t)r->esz();
    return check_channels("rs_process_stream", nouns, (size_t)r->n_channels, d_in, n_in, in_stride, isz, d_out, out_cap, out_stride, (size_t)r->esz(),
                          false);
}

// ---- integer-valued step: one of the kernels of the closed form
int rs_launch_fft(Rs *r, const RsCall &c, const PolyFftPlan *fp, long long K, bool can_fuse, bool *hist_fused)
{
    PolyFftArgs fa;
    memset(&fa, 0, sizeof(fa));
    fill_io(fa, r, c.io);
    fa.hist_out = can_fuse ? r->hist.next() : nullptr;
    *hist_fused = can_fuse;
    fa.H = fp->d_H;
    fa.tw = fp->d_tw;
    fa.n_out = K;
    fa.e_max = fp->e_max;
    fa.ovl = fp->Li - 1;
    fa.V = 256 - fa.ovl;
    fa.ticket = r->d_ticket;
    return launch_poly_fft(*fp, fa, r->data_complex, r->in_u8, r->n_channels, c.s);
}

int rs_launch_mfma(Rs *r, const RsCall &c, const PolyMfmaPlan *mp, long long K)
{
    PolyMfmaArgs ma;
    memset(&ma, 0, sizeof(ma));
    fill_io(ma, r, c.io);
    ma.A = mp->d_A;
    ma.n_out = K;
    ma.GS = mp->GS;
    ma.RG = mp->RG;
    ma.Kp = mp->Kp;
    ma.u_lo = mp->u_lo;
    return launch_poly_mfma(ma, r->n_channels, c.s);
}

// the generic kernel: any (step, pos0), float32 input
int rs_launch_int(Rs *r, const RsCall &c, const RsIntCall &ic)
{
    if (r->in_u8) {
        r->u8_refused = true;          // (the public entry converts the bytes and comes back with float32)
        set_error("rs_process_stream: u8 input needs a tiled kernel for this rate/tap shape");
        return SFE_ESTATE;
    }
    PolyArgs a = rs_poly_args(r, c.io);
    a.pos0 = ic.pos0;
    a.step = (int)c.stepf;
    a.n_out = ic.K;
    return launch_poly_int(a, r->data_complex, 0, r->exact_stream, r->n_channels, c.s);
}

// the tiled kernels, in the order they are tried: LDS-DMA runtime shape, compiled / runtime shape, the generic kernel
int rs_launch_tiled(Rs *r, const RsCall &c, const PolyTiledPlan *pl, const RsIntCall &ic, bool can_fuse, bool *hist_fused)
{
    PolyTiledArgs ta;
    fill_io(ta, r, c.io);
    ta.hist_out = can_fuse && !r->exact_stream ? r->hist.next() : nullptr;      // exact kernels: separate carry-over launch
    *hist_fused = ta.hist_out != nullptr;
    ta.G = pl->d_G;
    ta.Gt = pl->d_Gt;
    ta.n_out = ic.K;
    ta.Lp = pl->Lp;
    ta.e_max = pl->e_max;
    // shapes outside the compiled tables, float32 streams (complex or real), fused arithmetic: the tile by LDS-DMA, read in place (poly_rt_dma.hip)
    int rc = SFE_ESTATE;
    bool window_shape = !r->data_complex && poly_rt_dma_window_shape(pl->SP, pl->UP);      // real streams at small steps: the register-window kernel
#ifdef SFE_DIAG
    if (const char *e = getenv("SFE_RT_DMA_WINDOW")) window_shape = window_shape && pl->SP <= atoi(e);
#endif
    // wire-format input: four shapes have compile-time u8 kernels (/2, /4, /8, 5/3) and keep them; every other one -- the compile-time
    // float shapes included -- ran poly_rt_kernel's sample-by-sample byte loads (/7 0.71 ms where the float32 stream takes 0.45) and now
    // has its raw tile fetched by DMA and converted once (0.38 ms): profiles/r05/shapes_u8.txt
    const bool compiled = r->in_u8 ? poly_tiled_u8_is_compiled(pl->SP, pl->UP, pl->Lp) : poly_tiled_is_compiled(pl->SP, pl->UP, pl->Lp);
    bool try_dma = !r->exact_stream && (!compiled || window_shape);       // (real u8 streams at the window form's shapes: /2 0.72 -> 0.6 ms, profiles/r05/shapes_u8.txt)
#ifdef SFE_DIAG
    if (const char *e = getenv("SFE_RT_DMA_FORCE"))        // scripts/ab_dec8_dma.py: the LDS-DMA form also where a compile-time kernel exists
        if (atoi(e) && !r->exact_stream) try_dma = true;
    if (const char *e = getenv("SFE_RT_DMA_U8"))           // =0: wire-format input keeps poly_rt_kernel / the compile-time kernels (scripts/time_u8_shapes.py)
        if (!atoi(e) && r->in_u8) try_dma = false;
#endif
    if (try_dma) rc = launch_poly_rt_dma(*pl, ta, r->data_complex, r->in_u8, r->n_channels, c.s);
    if (rc == SFE_ESTATE && pl->UP <= 8) rc = launch_poly_tiled(*pl, ta, r->data_complex, r->exact_stream, r->in_u8, r->n_channels, c.s);
    if (rc == SFE_ESTATE && pl->UP > 8) {            // 9 ... 256 outputs per period and the tiled form declined: the generic kernel
        *hist_fused = false;
        rc = rs_launch_int(r, c, ic);
    }
    return rc;
}

int rs_run_int_step(Rs *r, const RsCall &c, size_t *n_out, bool *hist_fused)
{
    const long long S = (long long)c.stepf;
    const RsIntCall ic = rs_int_call(r->ts, r->U, (long long)c.n_in, S);
    const long long K = ic.K, pos0 = ic.pos0;
    if ((size_t)K > c.out_cap) {
        set_error("rs_process_stream: need room for %lld outputs, got %zu", K, c.out_cap);
        return SFE_ERANGE;
    }
    int rc = SFE_OK;
    // matrix-pipe form (fused numerics, cf32): opt-in with sfe_dsp_rs_set_algo(SFE_RS_ALGO_MFMA).  Measured slower
    // than the VALU kernel on the one shape where its tap matrix is dense (polyphase.hip).
    const PolyMfmaPlan *mp = nullptr;
    if (r->use_mfma && !r->exact_stream && r->data_complex && !r->in_u8) {
        mp = get_mfma_plan(r->mfma_plans, r->h_taps_pm, r->U, r->plen, (int)S, pos0, &rc);
        if (rc != SFE_OK) return rc;
    }
    // transform-domain form (fused numerics, cf32): long filters on streams long enough to fill the chip
    const PolyFftPlan *fp = nullptr;
    if (!mp && !r->exact_stream && K >= 4096) {
        fp = get_fft_plan(r->fft_plans, r->h_taps_pm, r->U, r->plen, (int)S, pos0, r->fft_mode, &rc);
        if (rc != SFE_OK) return rc;
    }
    const PolyTiledPlan *pl = (mp || fp) ? nullptr : get_tiled_plan(r->plans, r->h_taps_pm, r->U, r->plen, (int)S, pos0, &rc);
    if (rc != SFE_OK) return rc;
    // the transform-domain and the tiled kernels write the next call's history themselves (one launch per call)
    const bool can_fuse = c.n_in >= (size_t)r->hl && K > 0 && !c.capturing;
    if (fp) rc = rs_launch_fft(r, c, fp, K, can_fuse, hist_fused);
    else if (mp) rc = rs_launch_mfma(r, c, mp, K);
    else if (pl) rc = rs_launch_tiled(r, c, pl, ic, can_fuse, hist_fused);
    else rc = rs_launch_int(r, c, ic);
    if (rc != SFE_OK) return rc;
    r->ts = ic.after;
    *n_out = (size_t)K;
    return SFE_OK;
}

// ---- general rate: the plan (rs_plan.h), its upload, then the transform kernel, the direct kernel, the host schedule
// Plan tables: grow-only device arrays + pinned staging.  The previous call's UPLOADS may still be reading the
// staging: wait for them -- the event behind them -- not for the stream: that call's kernel runs on while this
// call is planned and queued (waiting for the stream here made every call a full host/device round trip).
// The device arrays themselves are ordered by the stream; a call on ANOTHER stream than the last waits for that one.
int rs_upload_plan(Rs *r, const RsPlan<SegChunk> &plan, hipStream_t s)
{
    int rc;
    if (r->ev_plan) {
        if (r->plan_stream != s) SFE_HIP(hipStreamSynchronize(r->plan_stream));
        else SFE_HIP(hipEventSynchronize(r->ev_plan));
    } else if ((rc = r->ev_plan.create()) != SFE_OK) {
        return rc;
    }
    const size_t n_table = plan.n_table, n_segs = plan.n_segs(), n_chunks = plan.chunks.size();
    if (n_segs > r->segs.cap) r->seg_uploaded = 0;          // regrown: the device holds nothing of the table
    if ((rc = r->segs.reserve(n_segs, n_segs * 2 + 1024)) != SFE_OK || (rc = r->chunks.reserve(n_chunks, n_chunks * 2 + 64)) != SFE_OK) return rc;
    // upload what the device does not hold yet: the table's new tail, then this call's own runs behind it
    TlSeg *hs = r->segs->h;
    const size_t from = r->seg_uploaded < n_table ? r->seg_uploaded : n_table;
    if (n_table > from) memcpy(hs + from, r->memo.table.data() + from, (n_table - from) * sizeof(TlSeg));
    if (!plan.extra.empty()) memcpy(hs + n_table, plan.extra.data(), plan.extra.size() * sizeof(TlSeg));
    if (n_segs > from)
        SFE_HIP(hipMemcpyAsync(r->segs->d.p + from, hs + from, (n_segs - from) * sizeof(TlSeg), hipMemcpyHostToDevice, s));
    r->seg_uploaded = n_table;
    memcpy(r->chunks->h, plan.chunks.data(), n_chunks * sizeof(SegChunk));
    SFE_HIP(hipMemcpyAsync(r->chunks->d, r->chunks->h, n_chunks * sizeof(SegChunk), hipMemcpyHostToDevice, s));
    SFE_HIP(hipEventRecord(r->ev_plan, s));
    r->plan_stream = s;
    return SFE_OK;
}

// Bulk calls (complex or real, float32 or u8) in fused arithmetic, at any rate: the transform-domain kernel (poly_gen.hip) --
// all U phases of every input by one forward and U inverse 4096-point transforms, outputs picked and blended from
// LDS by the same runs.  sfe_dsp_rs_set_algo(SFE_RS_ALGO_DIRECT) and the exact mode keep poly_seg_kernel.
// SFE_ESTATE: not a call for it (nothing launched).
int rs_launch_gen(Rs *r, const RsCall &c, const RsPlan<SegChunk> &plan)
{
    // (1 + U) transforms per block against two dot products of plen taps per output: the transform kernel while U <= 2 + plen / 16 (measured at
    // 2^26 samples and rate 1.77, profiles/r05/speed_sweep.txt: it takes 0.43 + 0.11 U ms, the direct kernel 0.69 + 0.0072 plen; until round 5
    // the rule was "12 taps per phase or more" and 16 phases of 127 taps ran 2.2 ms where the direct kernel takes 1.6)
    const bool gen_pays = r->plen >= 12 && r->U <= 2 + r->plen / 16;
    if (plan.exhausted || r->exact_stream || r->fft_mode < 0 ||
        !(r->fft_mode > 0 || r->in_u8 || (c.n_in >= ((size_t)1 << 16) && gen_pays)))
        return SFE_ESTATE;
    if (!r->gen_tried) {
        // spectra of the U phase filters (taps[i U + j], i < plen) from the FIR's table builder (fir_plan.h), one tap set per
        // phase, where the FIR planner serves a filter of plen + 1 taps -- one more, so that the overlap it picks covers plen
        // samples, not plen - 1 -- with one launch.  That one more tap is a zero: the spectra are those of the plen taps, and
        // h_taps_pm's rows are the sets as they lie.
        r->gen_tried = true;
        int ovl = 0, parts = 0;
        FirTables tab;
        if (fir_choose_partition(r->plen + 1, &ovl, &parts) && parts == 1 &&
            tab.upload(FirShape{r->plen, 0, r->U, 1, ovl}, r->h_taps_pm.data()) == SFE_OK)
            r->gen_tables = std::move(tab);
    }
    if (!r->gen_tables.hs) return SFE_ESTATE;
    const std::vector<SegChunk> &chunks = plan.chunks;
    PolyGenArgs ga;
    memset(&ga, 0, sizeof(ga));
    fill_io(ga, r, c.io);
    ga.hs = r->gen_tables.hs;
    ga.tw1 = r->gen_tables.tw1;
    ga.tw2 = r->gen_tables.tw2;
    ga.segs = r->segs->d;
    ga.chunks = r->chunks->d;
    ga.U = r->U;
    ga.plen = r->plen;
    ga.ovl = (r->plen + 15) & ~15;              // >= plen; the spectra do not depend on it
    ga.blksize = r->blksize;
    ga.n_chunks = (int)chunks.size();
    ga.real = r->data_complex ? 0 : 1;
    ga.in_u8 = r->in_u8 ? 1 : 0;
    int max_runs = 0;              // over any two (a real stream's pairs of blocks: three) consecutive calls
    for (size_t i = 0; i < chunks.size(); i++) {
        int sum = chunks[i].n_seg + (i + 1 < chunks.size() ? chunks[i + 1].n_seg : 0);
        if (ga.real && i + 2 < chunks.size()) sum += chunks[i + 2].n_seg;
        max_runs = sum > max_runs ? sum : max_runs;
    }
    return launch_poly_gen(ga, max_runs, c.stepf, r->n_channels, c.s);
}

// The direct kernel's LDS: a call larger than it is dealt to `split` workgroups, each tile sized by the largest input
// span any part of any call of this launch really reaches (segtile.h; rs_plan.h: rs_plan_max_span).  SFE_ESTATE: a part of a
// call reaches more input than the LDS holds, at any split (huge blksize).
int rs_launch_seg(Rs *r, const RsCall &c, const RsPlan<SegChunk> &plan)
{
    SegTilePlan tp;
    auto max_span = [&](int split) { return rs_plan_max_span(r->memo, plan, r->U, r->plen, split); };
    if (seg_tile_plan(r->U, r->plen, r->esz(), plan.max_m, max_span, &tp) != SFE_OK) return SFE_ESTATE;
    PolySegArgs sa;
    memset(&sa, 0, sizeof(sa));
    fill_io(sa, r, c.io);
    sa.taps = r->d_taps;
    sa.segs = r->segs->d;
    sa.chunks = r->chunks->d;
    sa.U = r->U;
    sa.plen = r->plen;
    sa.n_chunks = (int)plan.chunks.size();
    sa.max_m = plan.max_m;
    sa.split = tp.split;
    sa.tile_cap = tp.tile_cap;
    sa.taps_global = tp.taps_global;
    return launch_poly_seg(sa, r->data_complex, r->exact_stream, r->n_channels, c.s);
}

// the last resort: expand on the host and use the per-output schedule kernel
int rs_launch_sched(Rs *r, const RsCall &c, const RsPlan<SegChunk> &plan)
{
    const size_t K = plan.K;
    std::vector<long long> pos;
    std::vector<float> mu;
    rs_plan_expand(r->memo, plan, r->U, pos, mu);
    const int rc = rs_ensure_sched(r, K + 1);
    if (rc != SFE_OK) return rc;
    Rs::Sched &sc = r->sched.b;
    SFE_HIP(hipStreamSynchronize(c.s));        // the schedule staging may still be read by the previous call's uploads
    memcpy(sc.pos.h, pos.data(), K * sizeof(long long));
    memcpy(sc.mu.h, mu.data(), K * sizeof(float));
    SFE_HIP(hipMemcpyAsync(sc.pos.d, sc.pos.h, K * sizeof(long long), hipMemcpyHostToDevice, c.s));
    SFE_HIP(hipMemcpyAsync(sc.mu.d, sc.mu.h, K * sizeof(float), hipMemcpyHostToDevice, c.s));
    PolyArgs a = rs_poly_args(r, c.io);
    a.n_out = (long long)K;
    a.sched_pos = sc.pos.d;
    a.sched_mu = sc.mu.d;
    return launch_poly_sched(a, r->data_complex, r->exact_stream, r->n_channels, c.s);
}

int rs_run_general(Rs *r, const RsCall &c, size_t *n_out)
{
    // u8 input at a general rate: the transform-domain kernel converts on load (poly_gen.hip: IN_U8); the direct kernels
    // (exact mode, SFE_RS_ALGO_DIRECT) have no u8 form
    if (r->in_u8 && (r->exact_stream || r->fft_mode < 0)) {
        set_error("rs_process_stream: u8 input at a non-integer step runs the transform-domain kernel only (not the exact mode, not SFE_RS_ALGO_DIRECT)");
        return SFE_ESTATE;
    }
    const RsPlan<SegChunk> plan = rs_plan_calls<SegChunk>(r->memo, r->ts, r->U, r->blksize, c.n_in, c.rate);
    if (plan.memo_cleared) r->seg_uploaded = 0;
    if (plan.K > c.out_cap) {
        set_error("rs_process_stream: need room for %zu outputs, got %zu", plan.K, c.out_cap);
        return SFE_ERANGE;
    }
    int rc = rs_upload_plan(r, plan, c.s);
    if (rc != SFE_OK) return rc;
    rc = rs_launch_gen(r, c, plan);
    if (rc == SFE_ESTATE && r->in_u8) {
        r->u8_refused = true;              // (the public entry converts the bytes and comes back with float32)
        set_error("rs_process_stream: u8 input at a non-integer step: this call is outside what the transform-domain kernel takes "
                  "(more than 2032 taps per phase, more than 32 phases, blksize below a block's advance, or a call in the "
                  "reference's out_len-exhausted state)");
        return SFE_ESTATE;
    }
    if (rc == SFE_ESTATE) rc = rs_launch_seg(r, c, plan);
    if (rc == SFE_ESTATE) rc = rs_launch_sched(r, c, plan);
    if (rc != SFE_OK) return rc;
    r->ts = plan.after;
    *n_out = plan.K;
    return SFE_OK;
}

}  // namespace

static int rs_process_stream_impl(sfe_rs_t h, const void *d_in, size_t n_in, size_t in_stride,
                                  void *d_out, size_t out_cap, size_t out_stride, float rate,
                                  size_t *n_out, sfe_stream_t stream)
{
    Rs *r = as_rs(h);
    if (!r || !n_out) return SFE_EINVAL;
    *n_out = 0;
    int rc = rs_check_call(r, d_in, n_in, in_stride, d_out, out_cap, out_stride, rate);
    if (rc != SFE_OK || n_in == 0) return rc;
    SFE_ON_DEVICE(r->device);
    hipStream_t s = (hipStream_t)stream;
    const float stepf = rate * (float)r->U;
    const bool int_step = rs_int_step_law(stepf, r->ts, r->blksize, r->U);
    const RsCall c = {{d_in, d_out, (long long)n_in, (long long)in_stride, (long long)out_stride}, n_in, out_cap, rate, stepf, s, stream_is_capturing(s)};
    if (c.capturing && (!int_step || n_in < (size_t)r->hl || ((unsigned long long)n_in * (unsigned long long)r->U) % (unsigned long long)stepf != 0)) {
        set_error("rs_process_stream: a call captured into a hipGraph must leave the time state where it found it "
                  "(integer-valued step, n_in*upsample a multiple of it) and bring at least %d samples", r->hl);
        return SFE_ESTATE;
    }
    bool hist_fused = false;
    rc = int_step ? rs_run_int_step(r, c, n_out, &hist_fused) : rs_run_general(r, c, n_out);
    if (rc != SFE_OK) return rc;
    // (a captured call: the time state did not move)
    return carry_history(r->hist, r->captured, d_in, n_in, in_stride, r->hl, r->data_complex ? 2 : 1, r->n_channels, r->in_u8, hist_fused, c.capturing, s);
}

extern "C" {

// ---- cutting one stream into spans -------------------------
int sfe_dsp_rs_load_history(sfe_rs_t h, const void *d_prev, size_t n_prev, size_t stride, sfe_stream_t stream)
{
    return load_history("rs_load_history", as_rs(h), d_prev, n_prev, stride, (hipStream_t)stream);
}

int sfe_dsp_rs_get_state(sfe_rs_t h, sfe_rs_timestate *state)
{
    Rs *r = as_rs(h);
    if (!r || !state) return SFE_EINVAL;
    *state = r->ts;
    return SFE_OK;
}

int sfe_dsp_rs_set_state(sfe_rs_t h, const sfe_rs_timestate *state)
{
    Rs *r = as_rs(h);
    if (!r || !state || state->pos < -1 || !(state->mu >= 0.0f && state->mu < 1.0f)) {
        set_error("rs_set_state: need pos >= -1 and 0 <= mu < 1");
        return SFE_EINVAL;
    }
    r->ts = *state;
    r->ts.leftover = state->leftover ? 1 : 0;
    return SFE_OK;
}

// The time state a reference object has after consuming `first_sample` samples of a stream from a
// fresh start, in closed form -- only when fl(rate*upsample) is integer-valued (then mu == 0 and the
// float32 recurrence resample.cxx:129-150 is exact): output k sits at upsampled position k*S, the
// object's m_pos is the first such position at or after first_sample*U - 1, relative to it, and a
// position of exactly first_sample*U - 1 is the pending "leftover" output (resample.cxx:141-145).
int sfe_dsp_rs_plan_seek(sfe_rs_timestate *state, int upsample, uint64_t first_sample, float rate)
{
    if (!state || upsample < 1) return SFE_EINVAL;
    const float stepf = rate * (float)upsample;
    if (!rs_step_is_integer(stepf)) {
        set_error("rs_seek: fl(rate*upsample) = %g is not integer-valued: the float32 time recurrence has no closed form "
                  "(carry the state with sfe_dsp_rs_get_state / set_state instead)", (double)stepf);
        return SFE_ESTATE;
    }
    const unsigned long long S = (unsigned long long)stepf, U = (unsigned long long)upsample;
    if (first_sample == 0) {
        *state = {0, 0.0f, 0};
        return SFE_OK;
    }
    const unsigned long long edge = first_sample * U - 1;        // last upsampled position of the part before the cut
    const unsigned long long k = (edge + S - 1) / S;             // first output at or after it
    const long long rel = (long long)(k * S) - (long long)(first_sample * U);
    state->leftover = rel == -1 ? 1 : 0;
    state->pos = (int32_t)rel;
    state->mu = 0.0f;
    return SFE_OK;
}

int sfe_dsp_rs_seek(sfe_rs_t h, uint64_t first_sample, float rate)
{
    Rs *r = as_rs(h);
    if (!r) return SFE_EINVAL;
    return sfe_dsp_rs_plan_seek(&r->ts, r->U, first_sample, rate);
}

int sfe_dsp_rs_set_input_format(sfe_rs_t h, int fmt)
{
    Rs *r = as_rs(h);
    if (!r || (fmt != SFE_FMT_F32 && fmt != SFE_FMT_U8)) return SFE_EINVAL;
    if (r->piped && (fmt == SFE_FMT_U8) != (r->in_u8 != 0)) {
        set_error("rs_set_input_format: a pipe over this handle has frozen its item format (destroy the pipe first)");
        return SFE_ESTATE;
    }
    r->in_u8 = fmt == SFE_FMT_U8;
    return SFE_OK;
}

int sfe_dsp_rs_set_algo(sfe_rs_t h, int algo)
{
    Rs *r = as_rs(h);
    if (!r || algo < SFE_RS_ALGO_AUTO || algo > SFE_RS_ALGO_MFMA) return SFE_EINVAL;
    r->fft_mode = algo == SFE_RS_ALGO_FFT ? 1 : (algo == SFE_RS_ALGO_AUTO ? 0 : -1);
    r->use_mfma = algo == SFE_RS_ALGO_MFMA;
    // plans are cached per (step, pos0) together with the choice that made them; clearing frees
    // device tables a launch in flight may still read, so wait for the handle's device first, in
    // ITS context (the current device of a multi-GPU caller may be another one)
    SFE_ON_DEVICE(r->device);
    SFE_HIP(hipDeviceSynchronize());
    r->fft_plans.clear();
    return SFE_OK;
}

int sfe_dsp_rs_set_exact(sfe_rs_t h, int exact)
{
    Rs *r = as_rs(h);
    if (!r) return SFE_EINVAL;
    r->exact_stream = exact ? 1 : 0;
    return SFE_OK;
}

int sfe_dsp_rs_reset(sfe_rs_t h)
{
    Rs *r = as_rs(h);
    if (!r) return SFE_EINVAL;
    SFE_ON_DEVICE(r->device);
    SFE_HIP(hipDeviceSynchronize());
    const int rc = r->hist.zero();
    if (rc != SFE_OK) return rc;
    if (r->d_ticket) SFE_HIP(hipMemset(r->d_ticket, 0, POLY_TICKET_GROUPS * 128));
    r->ts.pos = 0;
    r->ts.mu = 0.0f;
    r->ts.leftover = 0;
    return SFE_OK;
}

int sfe_dsp_rs_destroy(sfe_rs_t h)
{
    Rs *r = as_rs(h);
    if (!r) return SFE_OK;
    if (r->piped) {
        set_error("rs_destroy: a pipe still borrows this handle (sfe_dsp_pipe_destroy first)");
        return SFE_ESTATE;
    }
    return destroy_handle(r);
}

}  // extern "C"
