// api_corr.hip -- the correlator-bank handle behind sfe_corr_t, sfe_dsp_corr_* (include/sfe_dsp.h).  Host code only; the
// kernels are in corr.hip.
#include <cmath>
#include <complex>

#include "host.h"
#include "block.h"

namespace sfe {

// corr.hip
int launch_corr(int u8, const void *in, long long in_stride, const v2f *hist, v2f *hist_next, const v2f *spec, const v2f *tpl,
                const v2f *tw, const float *energy, float *peak_val, unsigned *peak_idx, long long peak_stride, float *part_val, unsigned *part_idx,
                float *metric, long long metric_stride, long long n_in, int L, int K, int V, long long B, float min_energy,
                int n_streams, hipStream_t st);

namespace {

constexpr int CORR_FFT = 4096;

struct Corr {
    static constexpr uint32_t MAGIC = 0x434f5231u;   // 'COR1'
    uint32_t magic = MAGIC;
    int L = 0, K = 0, V = 0, ov = 0, B = 0, n_streams = 1, device = 0, in_u8 = 0;
    float min_energy = 0.0f;
    DevBuf<v2f> d_spec;             // [K][4096]: conj(DFT of conj(s_k) reversed) / 4096
    DevBuf<v2f> d_tpl;              // [K][L]: the templates themselves (the time-domain form of short templates)
    DevBuf<v2f> d_tw;               // [4096]: exp(-j 2 pi q / 4096)
    DevBuf<float> d_energy;         // [K]: E_k
    CarriedPair hist;               // the ov samples (cf32) before the next call, per stream
    GrowScratch part;               // the slot peaks of one call (B > V): values (float), then indices (unsigned)
    unsigned long long samples = 0; // per stream since create / reset
    size_t hist_bytes() const { return std::max<size_t>((size_t)n_streams * ov, 1) * sizeof(v2f); }
};

Corr *as_corr(void *h) { return as_handle<Corr>(h, "correlator"); }

int corr_check_shape(int L, int K, int B, int *advance)
{
    if (L < 1 || L > 2049) {
        set_error("corr: len = %d must be in [1, 2049]", L);
        return SFE_EINVAL;
    }
    if (K < 1 || K > 16) {
        set_error("corr: n_templates = %d must be in [1, 16]", K);
        return SFE_EINVAL;
    }
    const int V = CORR_FFT - 256 * ((L - 1 + 255) / 256);
    if (B < 1 || B % V) {
        set_error("corr: block = %d must be a positive multiple of the advance %d of len = %d", B, V, L);
        return SFE_EINVAL;
    }
    if (advance) *advance = V;
    return SFE_OK;
}

// in-place forward DFT of 4096 points in float64 (radix 2, decimation in time)
void corr_fft64(std::vector<std::complex<double>> &a)
{
    const int n = (int)a.size();
    for (int i = 1, j = 0; i < n; i++) {
        int bit = n >> 1;
        for (; j & bit; bit >>= 1) j ^= bit;
        j ^= bit;
        if (i < j) std::swap(a[i], a[j]);
    }
    for (int len = 2; len <= n; len <<= 1) {
        for (int i = 0; i < n; i += len) {
            for (int k = 0; k < len / 2; k++) {
                const double ang = -2.0 * M_PI * k / len;
                const std::complex<double> w(cos(ang), sin(ang)), u = a[i + k], v = a[i + k + len / 2] * w;
                a[i + k] = u + v;
                a[i + k + len / 2] = u - v;
            }
        }
    }
}

}  // namespace
}  // namespace sfe

using namespace sfe;

extern "C" {

int sfe_dsp_corr_plan(int len, int n_templates, int block, int *advance, int *history)
{
    int V = 0;
    const int rc = corr_check_shape(len, n_templates, block, &V);
    if (rc != SFE_OK) return rc;
    if (advance) *advance = V;
    if (history) *history = CORR_FFT - V;
    return SFE_OK;
}

int sfe_dsp_corr_create(const float *templates, int len, int n_templates, int block, float min_energy, int n_streams, int device,
                        sfe_corr_t *out)
{
    if (!out) return SFE_EINVAL;
    *out = nullptr;
    int V = 0;
    int rc = corr_check_shape(len, n_templates, block, &V);
    if (rc != SFE_OK) return rc;
    if (!templates || n_streams < 1) {
        set_error("corr: create needs templates and n_streams >= 1");
        return SFE_EINVAL;
    }
    if (!std::isfinite(min_energy) || min_energy < 0.0f) {
        set_error("corr: min_energy = %g must be finite and >= 0", (double)min_energy);
        return SFE_EINVAL;
    }
    // everything about the templates before the device is looked at: E_k in float64, rounded once
    std::vector<float> energy(n_templates);
    for (int k = 0; k < n_templates; k++) {
        double e = 0.0;
        for (int n = 0; n < 2 * len; n++) e += (double)templates[(size_t)k * 2 * len + n] * templates[(size_t)k * 2 * len + n];
        energy[k] = (float)e;
        if (!(energy[k] > 0.0f) || !std::isfinite(energy[k])) {
            set_error("corr: template %d has energy %g (an all-zero or non-finite template cannot be normalised)", k, e);
            return SFE_EINVAL;
        }
    }
    CreateScope scope(device);
    if (scope.rc != SFE_OK) return scope.rc;
    std::unique_ptr<Corr> p(new (std::nothrow) Corr);
    if (!p) return SFE_ENOMEM;
    p->L = len;
    p->K = n_templates;
    p->V = V;
    p->ov = CORR_FFT - V;
    p->B = block;
    p->min_energy = min_energy;
    p->n_streams = n_streams;
    p->device = device;
    // c_k = x convolved with h_k[n] = conj(s_k[L-1-n]); the kernel runs the inverse transform as a forward one of the
    // conjugated product, so it is handed conj(DFT h_k) / 4096
    std::vector<v2f> spec((size_t)n_templates * CORR_FFT);
    std::vector<std::complex<double>> h(CORR_FFT);
    for (int k = 0; k < n_templates; k++) {
        std::fill(h.begin(), h.end(), std::complex<double>(0.0, 0.0));
        const float *s = templates + (size_t)k * 2 * len;
        for (int n = 0; n < len; n++) h[n] = std::complex<double>(s[2 * (len - 1 - n)], -(double)s[2 * (len - 1 - n) + 1]);
        corr_fft64(h);
        for (int j = 0; j < CORR_FFT; j++)
            spec[(size_t)k * CORR_FFT + j] = v2f{(float)(h[j].real() / CORR_FFT), (float)(-h[j].imag() / CORR_FFT)};
    }
    if ((rc = p->d_spec.upload(spec)) != SFE_OK ||
        (rc = p->d_tpl.upload(reinterpret_cast<const v2f *>(templates), (size_t)n_templates * len)) != SFE_OK ||
        (rc = p->d_tw.upload(unit_circle(CORR_FFT, -1))) != SFE_OK || (rc = p->d_energy.upload(energy)) != SFE_OK ||
        (rc = p->hist.alloc_zero(p->hist_bytes())) != SFE_OK)
        return rc;
    SFE_HIP(hipDeviceSynchronize());
    *out = p.release();
    return SFE_OK;
}

int sfe_dsp_corr_set_input_format(sfe_corr_t h, int fmt)
{
    return set_format(as_corr(h), "corr_set_input_format", fmt, SFE_FMT_U8, "SFE_FMT_U8", &Corr::in_u8);
}

int sfe_dsp_corr_process_stream(sfe_corr_t h, const void *d_in, size_t n_in, size_t in_stride, void *d_peak_val, void *d_peak_idx,
                                size_t peak_stride, void *d_metric, size_t metric_stride, size_t *n_blocks, sfe_stream_t stream)
{
    static const char who[] = "corr_process_stream";
    Corr *p = stream_handle(as_corr(h), who, n_blocks, "n_blocks");
    if (!p) return SFE_EINVAL;
    if (n_in % (size_t)p->B) {
        set_error("corr_process_stream: n_in = %zu is not a multiple of block = %d", n_in, p->B);
        return SFE_EINVAL;
    }
    int rc = refuse_2_31(who, n_in);
    if (rc != SFE_OK) return rc;
    if (n_in == 0) return SFE_OK;
    const size_t blocks = n_in / p->B, rows = (size_t)p->n_streams * p->K;
    rc = refuse_null(who, {d_in, d_peak_val, d_peak_idx});
    if (rc != SFE_OK) return rc;
    if (peak_stride < blocks) {
        set_error("corr_process_stream: peak_stride %zu < n_blocks = %zu", peak_stride, blocks);
        return SFE_ERANGE;
    }
    if (d_metric && metric_stride < n_in) {
        set_error("corr_process_stream: metric_stride %zu < n_in = %zu", metric_stride, n_in);
        return SFE_ERANGE;
    }
    if (p->n_streams > 1 && in_stride < n_in) {
        set_error("corr_process_stream: in_stride %zu < n_in %zu with %d streams", in_stride, n_in, p->n_streams);
        return SFE_EINVAL;
    }
    CorrRanges r;
    if (!corr_ranges(p->n_streams, p->K, p->in_u8 ? 2 : 8, d_in, n_in, in_stride, d_peak_val, d_peak_idx, blocks, peak_stride, d_metric,
                     metric_stride, &r))
        return refuse_2_62(who);
    if ((rc = refuse_misaligned(who, "cf32 8 B, u8 (I,Q) pairs 2 B, outputs 4 B", {r.in, r.val, r.idx, r.met})) != SFE_OK ||
        (rc = refuse_overlap(who, r.in, {r.val, r.idx, r.met})) != SFE_OK ||
        (rc = refuse_outputs_overlap(who, {r.val, r.idx, r.met})) != SFE_OK)
        return rc;
    hipStream_t s = (hipStream_t)stream;
    rc = refuse_capture(who, "sample", s);
    if (rc != SFE_OK) return rc;
    SFE_ON_DEVICE(p->device);
    // B > V: the table of slot peaks grows when a larger call than any before arrives; with B = V there is none
    const size_t slots = n_in / p->V, need = p->B > p->V ? rows * slots : 0;
    rc = p->part.reserve(need * 8);
    if (rc != SFE_OK) return rc;
    float *part_val = p->part.as<float>();
    unsigned *part_idx = part_val ? reinterpret_cast<unsigned *>(part_val + p->part.bytes / 8) : nullptr;
    rc = launch_corr(p->in_u8, d_in, (long long)in_stride, p->hist.cur<v2f>(), p->hist.next<v2f>(), p->d_spec, p->d_tpl, p->d_tw,
                     p->d_energy, static_cast<float *>(d_peak_val), static_cast<unsigned *>(d_peak_idx), (long long)peak_stride, part_val,
                     part_idx, static_cast<float *>(d_metric), (long long)metric_stride, (long long)n_in, p->L, p->K, p->V,
                     (long long)p->B, p->min_energy, p->n_streams, s);
    if (rc != SFE_OK) return rc;
    p->hist.flip();
    p->samples += n_in;
    *n_blocks = blocks;
    return SFE_OK;
}

int sfe_dsp_corr_reset(sfe_corr_t h)
{
    Corr *p = as_corr(h);
    if (!p) return SFE_EINVAL;
    const int rc = reset_pairs(p->device, {&p->hist});
    if (rc == SFE_OK) p->samples = 0;
    return rc;
}

int sfe_dsp_corr_destroy(sfe_corr_t h) { return destroy_handle(as_corr(h)); }

}  // extern "C"
