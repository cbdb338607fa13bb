// api_ddc.hip -- the down-converter bank handle behind sfe_ddc_t, sfe_dsp_ddc_* (include/sfe_dsp.h).  Host code only; the
// kernels are in ddc.hip.
#include "host.h"
#include "block.h"

namespace sfe {

// ddc.hip
int ddc_tunings_per_chunk(int K);
int launch_ddc(int fmt, const void *in, long long in_stride, const void *hist, void *hist_next, const v2f *taps,
               const unsigned *inc, v2f *out, long long out_stride, long long n_in, int D, int P, int H, int K, int Kpad,
               unsigned c0, int n_streams, hipStream_t st);

namespace {

constexpr int DDC_RU = 4;       // tap rows per chunk of the kernel (ddc.hip): P is padded to a multiple of it

struct Ddc {
    static constexpr uint32_t MAGIC = 0x44444331u;   // 'DDC1'
    uint32_t magic = MAGIC;
    int D = 0, n_taps = 0, P = 0, Ppad = 0, H = 0, K = 0, Kpad = 0, KT = 1, n_streams = 1, device = 0, complex_in = 1, in_u8 = 0;
    std::vector<float> h;           // the prototype, for the tables of set_freqs
    DevBuf<v2f> d_taps;             // [Kpad / KT][Ppad][D][KT]: g_k[n] = h[n] exp(+j 2 pi phi_k(n) / 2^32), zero-padded
    DevBuf<uint32_t> d_inc;         // [Kpad]
    CarriedPair hist;               // [n_streams][H] each (cf32, or float for real input)
    unsigned long long count = 0;   // input samples per stream since create / reset
    size_t hist_bytes() const { return (size_t)n_streams * H * (complex_in ? sizeof(v2f) : sizeof(float)); }
};

Ddc *as_ddc(void *h) { return as_handle<Ddc>(h, "down-converter"); }

int ddc_check_freqs(int K, const double *freqs, uint32_t *inc)
{
    if (!freqs) {
        set_error("ddc: need %d frequencies", K);
        return SFE_EINVAL;
    }
    for (int k = 0; k < K; k++) {
        const double f = freqs[k];
        if (!(f >= -0.5 && f <= 0.5)) {            // NaN fails both
            set_error("ddc: frequency %d = %g is not in [-0.5, 0.5] cycles per sample", k, f);
            return SFE_EINVAL;
        }
        if (inc) inc[k] = (uint32_t)(uint64_t)llround(f * 4294967296.0);      // mod 2^32
    }
    return SFE_OK;
}

int ddc_check_shape(int n_taps, int D, int K)
{
    if (D < 1 || D > 1024) {
        set_error("ddc: decim = %d must be in [1, 1024]", D);
        return SFE_EINVAL;
    }
    if (n_taps < 1 || n_taps > 8192) {
        set_error("ddc: n_taps = %d must be in [1, 8192]", n_taps);
        return SFE_EINVAL;
    }
    if ((n_taps + D - 1) / D > 64) {
        set_error("ddc: n_taps = %d needs %d taps per branch at decim = %d; at most 64", n_taps, (n_taps + D - 1) / D, D);
        return SFE_EINVAL;
    }
    if (K < 1 || K > 64) {
        set_error("ddc: n_tunings = %d must be in [1, 64]", K);
        return SFE_EINVAL;
    }
    return SFE_OK;
}

// the kernel's tap table for increments inc[0..K): chunk-major, KT tunings interleaved per tap
std::vector<v2f> ddc_table(const Ddc *c, const uint32_t *inc)
{
    std::vector<v2f> t((size_t)c->Kpad * c->Ppad * c->D, v2f{0.0f, 0.0f});
    for (int k = 0; k < c->K; k++)
        for (int n = 0; n < c->n_taps; n++) {
            const uint32_t ph = (uint32_t)((uint64_t)n * inc[k]);                 // phi_k(n), exact
            const double a = 2.0 * M_PI * (double)(int32_t)ph / 4294967296.0;
            const int j = n / c->D, r = n % c->D, kc = k / c->KT, kk = k % c->KT;
            t[(((size_t)kc * c->Ppad + j) * c->D + r) * c->KT + kk] = v2f{(float)(c->h[n] * cos(a)), (float)(c->h[n] * sin(a))};
        }
    return t;
}

}  // namespace
}  // namespace sfe

using namespace sfe;

extern "C" {

int sfe_dsp_ddc_plan(int n_taps, int decim, int n_tunings, const double *freqs, int *taps_per_branch, int *history,
                     uint32_t *phase_inc)
{
    int rc = ddc_check_shape(n_taps, decim, n_tunings);
    if (rc != SFE_OK) return rc;
    rc = ddc_check_freqs(n_tunings, freqs, phase_inc);
    if (rc != SFE_OK) return rc;
    const int P = (n_taps + decim - 1) / decim;
    if (taps_per_branch) *taps_per_branch = P;
    if (history) *history = (P + DDC_RU - 1) / DDC_RU * DDC_RU * decim;
    return SFE_OK;
}

int sfe_dsp_ddc_create(const float *taps, int n_taps, int decim, int n_tunings, const double *freqs, int data_complex,
                       int n_streams, int device, sfe_ddc_t *out)
{
    if (!out) return SFE_EINVAL;
    *out = nullptr;
    int rc = ddc_check_shape(n_taps, decim, n_tunings);
    if (rc != SFE_OK) return rc;
    std::vector<uint32_t> inc(n_tunings);
    rc = ddc_check_freqs(n_tunings, freqs, inc.data());
    if (rc != SFE_OK) return rc;
    if (!taps || n_streams < 1 || n_streams > 65535) {
        set_error("ddc_create: need taps and 1 <= n_streams <= 65535");
        return SFE_EINVAL;
    }
    CreateScope scope(device);
    if (scope.rc != SFE_OK) return scope.rc;
    std::unique_ptr<Ddc> c(new (std::nothrow) Ddc);
    if (!c) return SFE_ENOMEM;
    c->D = decim;
    c->n_taps = n_taps;
    c->P = (n_taps + decim - 1) / decim;
    c->Ppad = (c->P + DDC_RU - 1) / DDC_RU * DDC_RU;
    c->H = c->Ppad * decim;
    c->K = n_tunings;
    c->KT = ddc_tunings_per_chunk(n_tunings);
    c->Kpad = (n_tunings + c->KT - 1) / c->KT * c->KT;
    c->n_streams = n_streams;
    c->device = device;
    c->complex_in = data_complex != 0;
    c->h.assign(taps, taps + n_taps);
    const std::vector<v2f> t = ddc_table(c.get(), inc.data());
    inc.resize(c->Kpad, 0u);
    if ((rc = c->d_taps.upload(t)) != SFE_OK || (rc = c->d_inc.upload(inc)) != SFE_OK || (rc = c->hist.alloc_zero(c->hist_bytes())) != SFE_OK)
        return rc;
    SFE_HIP(hipDeviceSynchronize());
    *out = c.release();
    return SFE_OK;
}

int sfe_dsp_ddc_set_input_format(sfe_ddc_t h, int fmt)
{
    Ddc *c = as_ddc(h);
    if (!c || (fmt != SFE_FMT_F32 && fmt != SFE_FMT_U8)) {
        set_error("ddc_set_input_format: null handle or a format other than SFE_FMT_F32 / SFE_FMT_U8");
        return SFE_EINVAL;
    }
    if (fmt == SFE_FMT_U8 && !c->complex_in) {
        set_error("ddc_set_input_format: u8 input is (I,Q) pairs; this handle takes real data");
        return SFE_EINVAL;
    }
    c->in_u8 = fmt == SFE_FMT_U8;
    return SFE_OK;
}

int sfe_dsp_ddc_set_freqs(sfe_ddc_t h, const double *freqs)
{
    Ddc *c = as_ddc(h);
    if (!c) return SFE_EINVAL;
    std::vector<uint32_t> inc(c->K);
    const int rc = ddc_check_freqs(c->K, freqs, inc.data());
    if (rc != SFE_OK) return rc;
    const std::vector<v2f> t = ddc_table(c, inc.data());
    inc.resize(c->Kpad, 0u);
    SFE_ON_DEVICE(c->device);
    // calls already enqueued read the tables: they finish with the old ones before these are replaced
    SFE_HIP(hipDeviceSynchronize());
    SFE_HIP(hipMemcpy(c->d_taps, t.data(), t.size() * sizeof(v2f), hipMemcpyHostToDevice));
    SFE_HIP(hipMemcpy(c->d_inc, inc.data(), inc.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    SFE_HIP(hipDeviceSynchronize());
    return SFE_OK;
}

int sfe_dsp_ddc_process_stream(sfe_ddc_t h, const void *d_in, size_t n_in, size_t in_stride, void *d_out, size_t out_stride,
                               size_t *n_out, sfe_stream_t stream)
{
    static const char who[] = "ddc_process_stream";
    Ddc *c = stream_handle(as_ddc(h), who, n_out);
    if (!c) return SFE_EINVAL;
    if (n_in % (size_t)c->D) {
        set_error("ddc_process_stream: n_in = %zu is not a multiple of decim = %d", n_in, c->D);
        return SFE_EINVAL;
    }
    static const StreamNouns nouns{"n_out ", "cf32 8 B, real float 4 B, u8 (I,Q) pairs 2 B", true, true};
    const size_t no = n_in / c->D;
    bool go;
    int rc = check_streams(who, nouns, d_in, n_in, in_stride, c->n_streams, c->in_u8 ? 2 : c->complex_in ? 8 : 4, d_out, out_stride, no,
                           (size_t)c->n_streams * c->K, sizeof(v2f), &go);
    if (rc != SFE_OK || !go) return rc;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = refuse_capture(who, "sample", s)) != SFE_OK) return rc;       // the lead factors' phase
    SFE_ON_DEVICE(c->device);
    const int fmt = c->in_u8 ? 1 : c->complex_in ? 0 : 2;
    rc = launch_ddc(fmt, d_in, (long long)in_stride, c->hist.cur<void>(), c->hist.next<void>(), c->d_taps, c->d_inc,
                    static_cast<v2f *>(d_out), (long long)out_stride, (long long)n_in, c->D, c->Ppad, c->H, c->K, c->Kpad,
                    (unsigned)(c->count & 0xffffffffu), c->n_streams, s);
    if (rc != SFE_OK) return rc;
    c->hist.flip();
    c->count += n_in;
    *n_out = no;
    return SFE_OK;
}

int sfe_dsp_ddc_reset(sfe_ddc_t h)
{
    Ddc *c = as_ddc(h);
    if (!c) return SFE_EINVAL;
    const int rc = reset_pairs(c->device, {&c->hist});
    if (rc == SFE_OK) c->count = 0;
    return rc;
}

int sfe_dsp_ddc_destroy(sfe_ddc_t h) { return destroy_handle(as_ddc(h)); }

}  // extern "C"
