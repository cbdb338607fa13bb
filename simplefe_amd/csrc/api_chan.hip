// api_chan.hip -- the channelizer handle behind sfe_chan_t, sfe_dsp_chan_* (include/sfe_dsp.h).  Host code only; the
// kernels are in chan.hip.
#include "host.h"
#include "block.h"

namespace sfe {

// chan.hip
int chan_tile_rows(int logm);
int launch_chan(int logm, int half, int u8, const void *in, long long in_stride, const v2f *hist, v2f *hist_next,
                const float *taps, const v2f *tw, v2f *out, long long out_stride, long long n_in, long long n_out, int P, int H,
                int parity, int n_streams, hipStream_t st);

namespace {

constexpr int CHAN_RU = 8;      // tap rows per chunk of the kernel (chan.hip): P is padded to a multiple of it

struct Chan {
    static constexpr uint32_t MAGIC = 0x43484e31u;   // 'CHN1'
    uint32_t magic = MAGIC;
    int M = 0, logm = 0, D = 0, n_taps = 0, P = 0, Ppad = 0, H = 0, n_streams = 1, device = 0, in_u8 = 0;
    DevBuf<float> d_taps;           // [Ppad][M]: h zero-padded
    DevBuf<v2f> d_tw;               // [M]: exp(+j 2 pi q / M)
    CarriedPair hist;               // [n_streams][H] cf32 each
    unsigned long long m_count = 0; // outputs per channel since create / reset
    size_t hist_bytes() const { return (size_t)n_streams * H * sizeof(v2f); }
};

Chan *as_chan(void *h) { return as_handle<Chan>(h, "channelizer"); }

int chan_check_shape(int n_taps, int M, int D, int *logm)
{
    int lg = 0;
    while (lg < 30 && (1 << lg) < M) lg++;
    if (M < 4 || M > 1024 || (1 << lg) != M) {
        set_error("chan: n_chans = %d must be a power of two in [4, 1024]", M);
        return SFE_EINVAL;
    }
    if (D != M && D != M / 2) {
        set_error("chan: decim = %d must be n_chans (%d) or n_chans / 2 (%d)", D, M, M / 2);
        return SFE_EINVAL;
    }
    if (n_taps < 1 || n_taps > 32 * M) {
        set_error("chan: n_taps = %d must be in [1, 32 * n_chans = %d]", n_taps, 32 * M);
        return SFE_EINVAL;
    }
    if (logm) *logm = lg;
    return SFE_OK;
}

}  // namespace
}  // namespace sfe

using namespace sfe;

extern "C" {

int sfe_dsp_chan_plan(int n_taps, int n_chans, int decim, int *taps_per_branch, int *history)
{
    const int rc = chan_check_shape(n_taps, n_chans, decim, nullptr);
    if (rc != SFE_OK) return rc;
    const int P = (n_taps + n_chans - 1) / n_chans;
    if (taps_per_branch) *taps_per_branch = P;
    if (history) *history = (P + CHAN_RU - 1) / CHAN_RU * CHAN_RU * n_chans;
    return SFE_OK;
}

int sfe_dsp_chan_create(const float *taps, int n_taps, int n_chans, int decim, int n_streams, int device, sfe_chan_t *out)
{
    if (!out) return SFE_EINVAL;
    *out = nullptr;
    int logm = 0;
    int rc = chan_check_shape(n_taps, n_chans, decim, &logm);
    if (rc != SFE_OK) return rc;
    if (!taps || n_streams < 1) {
        set_error("chan_create: need taps and n_streams >= 1");
        return SFE_EINVAL;
    }
    CreateScope scope(device);
    if (scope.rc != SFE_OK) return scope.rc;
    std::unique_ptr<Chan> c(new (std::nothrow) Chan);
    if (!c) return SFE_ENOMEM;
    c->M = n_chans;
    c->logm = logm;
    c->D = decim;
    c->n_taps = n_taps;
    c->P = (n_taps + n_chans - 1) / n_chans;
    c->Ppad = (c->P + CHAN_RU - 1) / CHAN_RU * CHAN_RU;
    c->H = c->Ppad * n_chans;
    c->n_streams = n_streams;
    c->device = device;
    std::vector<float> hp((size_t)c->Ppad * n_chans, 0.0f);
    std::copy(taps, taps + n_taps, hp.begin());
    if ((rc = c->d_taps.upload(hp)) != SFE_OK || (rc = c->d_tw.upload(unit_circle(n_chans, +1))) != SFE_OK ||
        (rc = c->hist.alloc_zero(c->hist_bytes())) != SFE_OK)
        return rc;
    SFE_HIP(hipDeviceSynchronize());
    *out = c.release();
    return SFE_OK;
}

int sfe_dsp_chan_set_input_format(sfe_chan_t h, int fmt)
{
    return set_format(as_chan(h), "chan_set_input_format", fmt, SFE_FMT_U8, "SFE_FMT_U8", &Chan::in_u8);
}

int sfe_dsp_chan_process_stream(sfe_chan_t h, const void *d_in, size_t n_in, size_t in_stride, void *d_out, size_t out_stride,
                                size_t *n_out, sfe_stream_t stream)
{
    static const char who[] = "chan_process_stream";
    Chan *c = stream_handle(as_chan(h), who, n_out);
    if (!c) return SFE_EINVAL;
    if (n_in % (size_t)c->D) {
        set_error("chan_process_stream: n_in = %zu is not a multiple of decim = %d", n_in, c->D);
        return SFE_EINVAL;
    }
    static const StreamNouns nouns{"n_out ", "cf32 8 B, u8 (I,Q) pairs 2 B", false, true};
    const size_t no = n_in / c->D;
    bool go;
    int rc = check_streams(who, nouns, d_in, n_in, in_stride, c->n_streams, c->in_u8 ? 2 : 8, d_out, out_stride, no,
                           (size_t)c->n_streams * c->M, sizeof(v2f), &go);
    if (rc != SFE_OK || !go) return rc;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = refuse_capture(who, "output", s)) != SFE_OK) return rc;       // the counter: the D = M/2 parity
    SFE_ON_DEVICE(c->device);
    rc = launch_chan(c->logm, c->D != c->M, c->in_u8, d_in, (long long)in_stride, c->hist.cur<v2f>(), c->hist.next<v2f>(), c->d_taps,
                     c->d_tw, static_cast<v2f *>(d_out), (long long)out_stride, (long long)n_in, (long long)no, c->Ppad, c->H,
                     (int)(c->m_count & 1), c->n_streams, s);
    if (rc != SFE_OK) return rc;
    c->hist.flip();
    c->m_count += no;
    *n_out = no;
    return SFE_OK;
}

int sfe_dsp_chan_reset(sfe_chan_t h)
{
    Chan *c = as_chan(h);
    if (!c) return SFE_EINVAL;
    const int rc = reset_pairs(c->device, {&c->hist});
    if (rc == SFE_OK) c->m_count = 0;
    return rc;
}

int sfe_dsp_chan_destroy(sfe_chan_t h) { return destroy_handle(as_chan(h)); }

}  // extern "C"
