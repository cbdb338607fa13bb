// api_combine.hip -- the synthesis filter bank handle behind sfe_combine_t, sfe_dsp_combine_* (include/sfe_dsp.h).  Host
// code only; the kernels are in combine.hip.
#include "host.h"
#include "block.h"

namespace sfe {

// combine.hip
int combine_segments(int logm, int half, int logj);
int combine_chunk_rows(int logm, int half, int logj);
int launch_combine(int logm, int half, int logj, int tx10, const v2f *in, long long in_stride, const v2f *hist, v2f *hist_next,
                   const float *taps, const v2f *tw, void *out, long long out_stride, long long n_in, long long run, int Hr,
                   int parity, int n_streams, hipStream_t st);

namespace {

struct Combiner {
    static constexpr uint32_t MAGIC = 0x434d4231u;   // 'CMB1'
    uint32_t magic = MAGIC;
    int M = 0, logm = 0, D = 0, n_taps = 0, P = 0, logj = 0, Hr = 0, n_streams = 1, device = 0, out_tx10 = 0;
    DevBuf<float> d_taps;           // [J][D]: g zero-padded
    DevBuf<v2f> d_tw;               // [M]: exp(+j 2 pi q / M)
    CarriedPair hist;               // [n_streams][M][Hr] cf32 each
    unsigned long long m_count = 0; // instants since create / reset
    size_t hist_bytes() const { return (size_t)n_streams * M * Hr * sizeof(v2f); }
};

Combiner *as_combiner(void *h) { return as_handle<Combiner>(h, "combiner"); }

// P = ceil(L / D) taps per output phase; the kernel's delay line is J = the power of two >= max(8, P) long
int combine_check_shape(int n_taps, int M, int D, int *logm, int *P, int *logj)
{
    int lg = 0;
    while (lg < 30 && (1 << lg) < M) lg++;
    if (M < 4 || M > 1024 || (1 << lg) != M) {
        set_error("combine: n_chans = %d must be a power of two in [4, 1024]", M);
        return SFE_EINVAL;
    }
    if (D != M && D != M / 2) {
        set_error("combine: interp = %d must be n_chans (%d) or n_chans / 2 (%d)", D, M, M / 2);
        return SFE_EINVAL;
    }
    if (n_taps < 1 || n_taps > 32 * M) {
        set_error("combine: n_taps = %d must be in [1, 32 * n_chans = %d]", n_taps, 32 * M);
        return SFE_EINVAL;
    }
    const int p = (n_taps + D - 1) / D;
    int lj = 3;
    while ((1 << lj) < p) lj++;
    if (logm) *logm = lg;
    if (P) *P = p;
    if (logj) *logj = lj;
    return SFE_OK;
}

}  // namespace
}  // namespace sfe

using namespace sfe;

extern "C" {

int sfe_dsp_combine_plan(int n_taps, int n_chans, int interp, int *taps_per_branch, int *history)
{
    int P = 0, logj = 0;
    const int rc = combine_check_shape(n_taps, n_chans, interp, nullptr, &P, &logj);
    if (rc != SFE_OK) return rc;
    if (taps_per_branch) *taps_per_branch = P;
    if (history) *history = (1 << logj) - 1;
    return SFE_OK;
}

int sfe_dsp_combine_create(const float *taps, int n_taps, int n_chans, int interp, int n_streams, int device, sfe_combine_t *out)
{
    if (!out) return SFE_EINVAL;
    *out = nullptr;
    int logm = 0, P = 0, logj = 0;
    int rc = combine_check_shape(n_taps, n_chans, interp, &logm, &P, &logj);
    if (rc != SFE_OK) return rc;
    if (!taps || n_streams < 1) {
        set_error("combine_create: need taps and n_streams >= 1");
        return SFE_EINVAL;
    }
    CreateScope scope(device);
    if (scope.rc != SFE_OK) return scope.rc;
    std::unique_ptr<Combiner> c(new (std::nothrow) Combiner);
    if (!c) return SFE_ENOMEM;
    c->M = n_chans;
    c->logm = logm;
    c->D = interp;
    c->n_taps = n_taps;
    c->P = P;
    c->logj = logj;
    c->Hr = (1 << logj) - 1;
    c->n_streams = n_streams;
    c->device = device;
    std::vector<float> gp((size_t)interp << logj, 0.0f);
    std::copy(taps, taps + n_taps, gp.begin());
    if ((rc = c->d_taps.upload(gp)) != SFE_OK || (rc = c->d_tw.upload(unit_circle(n_chans, +1))) != SFE_OK ||
        (rc = c->hist.alloc_zero(c->hist_bytes())) != SFE_OK)
        return rc;
    SFE_HIP(hipDeviceSynchronize());
    *out = c.release();
    return SFE_OK;
}

int sfe_dsp_combine_set_output_format(sfe_combine_t h, int fmt)
{
    return set_format(as_combiner(h), "combine_set_output_format", fmt, SFE_FMT_TX10, "SFE_FMT_TX10", &Combiner::out_tx10);
}

int sfe_dsp_combine_process_stream(sfe_combine_t h, const void *d_in, size_t n_in, size_t in_stride, void *d_out, size_t out_stride,
                                   size_t *n_out, sfe_stream_t stream)
{
    static const char who[] = "combine_process_stream";
    Combiner *c = stream_handle(as_combiner(h), who, n_out);
    if (!c) return SFE_EINVAL;
    if (n_in == 0) return SFE_OK;
    const size_t no = n_in * (size_t)c->D;
    int rc = refuse_null(who, {d_in, d_out});
    if (rc != SFE_OK) return rc;
    if (out_stride < no) {
        set_error("combine_process_stream: out_stride %zu < n_out %zu", out_stride, no);
        return SFE_ERANGE;
    }
    if (in_stride < n_in) {
        set_error("combine_process_stream: in_stride %zu < n_in %zu", in_stride, n_in);
        return SFE_EINVAL;
    }
    if (c->out_tx10 && (out_stride & 1)) {
        set_error("combine_process_stream: out_stride %zu must be even with SFE_FMT_TX10 (whole 5-byte groups per stream)", out_stride);
        return SFE_EINVAL;
    }
    Span in, out;
    if (!combine_ranges(c->n_streams, c->M, c->out_tx10, d_in, n_in, in_stride, d_out, no, out_stride, &in, &out)) return refuse_2_62(who);
    rc = refuse_misaligned(who, "cf32 8 B", {in, out});
    if (rc != SFE_OK) return rc;
    // the kernel indexes within one stream in 32 bits
    if ((size_t)(c->M - 1) * in_stride + n_in >= (1ull << 31) || no >= (1ull << 31)) {
        set_error("combine_process_stream: a stream's input (%d x %zu) or output (%zu) reaches 2^31 samples", c->M, in_stride, no);
        return SFE_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    if ((rc = refuse_overlap(who, in, {out})) != SFE_OK || (rc = refuse_capture(who, "instant", s)) != SFE_OK)   // the D = M/2 parity
        return rc;
    SFE_ON_DEVICE(c->device);
    // instants per segment: whole chunks, long enough that the J - 1 warm-up rows stay a small part of the work, and
    // short enough to give every compute unit several workgroups
    const long long rg = combine_chunk_rows(c->logm, c->D != c->M, c->logj);
    const long long segs = combine_segments(c->logm, c->D != c->M, c->logj);
    const long long want_wg = 8LL * device_cu_count();
    long long run = ((long long)n_in * c->n_streams + want_wg * segs - 1) / (want_wg * segs);
    run = std::max(run, 4LL * (1 << c->logj));
    run = std::min(run, (long long)n_in);
    run = (run + rg - 1) / rg * rg;
    rc = launch_combine(c->logm, c->D != c->M, c->logj, c->out_tx10, static_cast<const v2f *>(d_in), (long long)in_stride,
                        c->hist.cur<v2f>(), c->hist.next<v2f>(), c->d_taps, c->d_tw, d_out, (long long)out_stride, (long long)n_in, run,
                        c->Hr, (int)(c->m_count & 1), c->n_streams, s);
    if (rc != SFE_OK) return rc;
    c->hist.flip();
    c->m_count += n_in;
    *n_out = no;
    return SFE_OK;
}

int sfe_dsp_combine_reset(sfe_combine_t h)
{
    Combiner *c = as_combiner(h);
    if (!c) return SFE_EINVAL;
    const int rc = reset_pairs(c->device, {&c->hist});
    if (rc == SFE_OK) c->m_count = 0;
    return rc;
}

int sfe_dsp_combine_destroy(sfe_combine_t h) { return destroy_handle(as_combiner(h)); }

}  // extern "C"
