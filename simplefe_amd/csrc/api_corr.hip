// api_corr.hip -- the correlator-bank handle behind sfe_corr_t, sfe_dsp_corr_* (include/sfe_dsp.h).  Host code only; the
// kernels are in corr.hip.
#include <cmath>
#include <complex>

#include "host.h"

namespace sfe {

// corr.hip
int launch_corr(int u8, const void *in, long long in_stride, const v2f *hist, v2f *hist_next, const v2f *spec, const v2f *tpl,
                const v2f *tw, const float *energy, float *peak_val, unsigned *peak_idx, long long peak_stride, float *part_val, unsigned *part_idx,
                float *metric, long long metric_stride, long long n_in, int L, int K, int V, long long B, float min_energy,
                int n_streams, hipStream_t st);

namespace {

constexpr int CORR_FFT = 4096;

struct Corr {
    uint32_t magic = 0x434f5231u;   // 'COR1'
    int L = 0, K = 0, V = 0, ov = 0, B = 0, n_streams = 1, device = 0, in_u8 = 0;
    float min_energy = 0.0f;
    v2f *d_spec = nullptr;          // [K][4096]: conj(DFT of conj(s_k) reversed) / 4096
    v2f *d_tpl = nullptr;           // [K][L]: the templates themselves (the time-domain form of short templates)
    v2f *d_tw = nullptr;            // [4096]: exp(-j 2 pi q / 4096)
    float *d_energy = nullptr;      // [K]: E_k
    v2f *d_hist[2] = {nullptr, nullptr};    // the ov samples before the next call, per stream: the current one and the next call's
    int cur = 0;
    void *d_part = nullptr;         // the slot peaks of one call (B > V): values, then indices; grows with the largest call seen
    size_t part_slots = 0;
    unsigned long long samples = 0; // per stream since create / reset
    size_t hist_bytes() const { return std::max<size_t>((size_t)n_streams * ov, 1) * sizeof(v2f); }
};

Corr *as_corr(void *h)
{
    Corr *p = static_cast<Corr *>(h);
    if (p && p->magic != 0x434f5231u) {
        set_error("not a live correlator handle");
        return nullptr;
    }
    return p;
}

void corr_free(Corr *p)
{
    if (!p) return;
    if (p->d_spec) (void)hipFree(p->d_spec);
    if (p->d_tpl) (void)hipFree(p->d_tpl);
    if (p->d_tw) (void)hipFree(p->d_tw);
    if (p->d_energy) (void)hipFree(p->d_energy);
    if (p->d_part) (void)hipFree(p->d_part);
    for (int i = 0; i < 2; i++)
        if (p->d_hist[i]) (void)hipFree(p->d_hist[i]);
    p->magic = 0;
    delete p;
}

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
    int prev_dev = -1;
    (void)hipGetDevice(&prev_dev);
    rc = use_device(device);
    if (rc != SFE_OK) return rc;
    struct Restore { int d; ~Restore() { if (d >= 0) (void)hipSetDevice(d); } } restore__{prev_dev};
    Corr *p = new (std::nothrow) Corr;
    if (!p) return SFE_ENOMEM;
    p->L = len;
    p->K = n_templates;
    p->V = V;
    p->ov = CORR_FFT - V;
    p->B = block;
    p->min_energy = min_energy;
    p->n_streams = n_streams;
    p->device = device;
    auto fail = [&](int code) { corr_free(p); return code; };
#define TRY(call) do { hipError_t e__ = (call); if (e__ != hipSuccess) return fail(hip_fail(e__, #call)); } while (0)
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
    std::vector<v2f> tw(CORR_FFT);
    for (int q = 0; q < CORR_FFT; q++) {
        const double a = 2.0 * M_PI * q / CORR_FFT;
        tw[q] = v2f{(float)cos(a), (float)-sin(a)};
        if (q % (CORR_FFT / 4) == 0) {      // the quarter turns exactly
            static const float cq[4] = {1.0f, 0.0f, -1.0f, 0.0f}, sq[4] = {0.0f, -1.0f, 0.0f, 1.0f};
            tw[q] = v2f{cq[q / (CORR_FFT / 4)], sq[q / (CORR_FFT / 4)]};
        }
    }
    TRY(hipMalloc(&p->d_spec, spec.size() * sizeof(v2f)));
    TRY(hipMemcpy(p->d_spec, spec.data(), spec.size() * sizeof(v2f), hipMemcpyHostToDevice));
    TRY(hipMalloc(&p->d_tpl, (size_t)n_templates * len * sizeof(v2f)));
    TRY(hipMemcpy(p->d_tpl, templates, (size_t)n_templates * len * sizeof(v2f), hipMemcpyHostToDevice));
    TRY(hipMalloc(&p->d_tw, tw.size() * sizeof(v2f)));
    TRY(hipMemcpy(p->d_tw, tw.data(), tw.size() * sizeof(v2f), hipMemcpyHostToDevice));
    TRY(hipMalloc(&p->d_energy, energy.size() * sizeof(float)));
    TRY(hipMemcpy(p->d_energy, energy.data(), energy.size() * sizeof(float), hipMemcpyHostToDevice));
    for (int i = 0; i < 2; i++) {
        TRY(hipMalloc(&p->d_hist[i], p->hist_bytes()));
        TRY(hipMemset(p->d_hist[i], 0, p->hist_bytes()));
    }
    TRY(hipDeviceSynchronize());
#undef TRY
    *out = p;
    return SFE_OK;
}

int sfe_dsp_corr_set_input_format(sfe_corr_t h, int fmt)
{
    Corr *p = as_corr(h);
    if (!p || (fmt != SFE_FMT_F32 && fmt != SFE_FMT_U8)) {
        set_error("corr_set_input_format: null handle or a format other than SFE_FMT_F32 / SFE_FMT_U8");
        return SFE_EINVAL;
    }
    p->in_u8 = fmt == SFE_FMT_U8;
    return SFE_OK;
}

int sfe_dsp_corr_process_stream(sfe_corr_t h, const void *d_in, size_t n_in, size_t in_stride, void *d_peak_val, void *d_peak_idx,
                                size_t peak_stride, void *d_metric, size_t metric_stride, size_t *n_blocks, sfe_stream_t stream)
{
    Corr *p = as_corr(h);
    if (n_blocks) *n_blocks = 0;
    if (!p || !n_blocks) {
        set_error("corr_process_stream: null handle or n_blocks");
        return SFE_EINVAL;
    }
    if (n_in % (size_t)p->B) {
        set_error("corr_process_stream: n_in = %zu is not a multiple of block = %d", n_in, p->B);
        return SFE_EINVAL;
    }
    if (n_in >= ((size_t)1 << 31)) {
        set_error("corr_process_stream: n_in = %zu must be below 2^31", n_in);
        return SFE_EINVAL;
    }
    if (n_in == 0) return SFE_OK;
    const size_t blocks = n_in / p->B, rows = (size_t)p->n_streams * p->K;
    if (!d_in || !d_peak_val || !d_peak_idx) {
        set_error("corr_process_stream: null buffer");
        return SFE_EINVAL;
    }
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
    const size_t isz = p->in_u8 ? 2 : 8;
    if ((reinterpret_cast<uintptr_t>(d_in) & (isz - 1)) || (reinterpret_cast<uintptr_t>(d_peak_val) & 3) ||
        (reinterpret_cast<uintptr_t>(d_peak_idx) & 3) || (reinterpret_cast<uintptr_t>(d_metric) & 3)) {
        set_error("corr_process_stream: buffers must be aligned to their element (cf32 8 B, u8 (I,Q) pairs 2 B, outputs 4 B)");
        return SFE_EINVAL;
    }
    const size_t in_b = ((size_t)(p->n_streams - 1) * in_stride + n_in) * isz;
    const size_t peak_b = ((rows - 1) * peak_stride + blocks) * 4;
    const size_t met_b = d_metric ? ((rows - 1) * metric_stride + n_in) * 4 : 0;
    if (ranges_overlap(d_in, in_b, d_peak_val, peak_b) || ranges_overlap(d_in, in_b, d_peak_idx, peak_b) ||
        (met_b && ranges_overlap(d_in, in_b, d_metric, met_b))) {
        set_error("corr_process_stream: input and output ranges overlap (in-place operation is not supported)");
        return SFE_EINVAL;
    }
    if (ranges_overlap(d_peak_val, peak_b, d_peak_idx, peak_b) ||
        (met_b && (ranges_overlap(d_metric, met_b, d_peak_val, peak_b) || ranges_overlap(d_metric, met_b, d_peak_idx, peak_b)))) {
        set_error("corr_process_stream: the output ranges overlap one another");
        return SFE_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    if (stream_is_capturing(s)) {
        // the sample counter and the history pair advance on the host
        set_error("corr_process_stream: graph capture is not supported (the sample counter lives on the host)");
        return SFE_ESTATE;
    }
    SFE_ON_DEVICE(p->device);
    // B > V: the table of slot peaks grows when a larger call than any before arrives; with B = V there is none
    const size_t slots = n_in / p->V, need = p->B > p->V ? rows * slots : 0;
    if (need > p->part_slots) {
        SFE_HIP(hipDeviceSynchronize());
        if (p->d_part) (void)hipFree(p->d_part);
        p->d_part = nullptr;
        p->part_slots = 0;
        SFE_HIP(hipMalloc(&p->d_part, need * 8));
        p->part_slots = need;
    }
    const int c = p->cur;
    float *part_val = static_cast<float *>(p->d_part);
    unsigned *part_idx = p->d_part ? reinterpret_cast<unsigned *>(part_val + p->part_slots) : nullptr;
    const int rc = launch_corr(p->in_u8, d_in, (long long)in_stride, p->d_hist[c], p->d_hist[c ^ 1], p->d_spec, p->d_tpl, p->d_tw, p->d_energy,
                               static_cast<float *>(d_peak_val), static_cast<unsigned *>(d_peak_idx), (long long)peak_stride, part_val,
                               part_idx, static_cast<float *>(d_metric), (long long)metric_stride, (long long)n_in, p->L, p->K, p->V,
                               (long long)p->B, p->min_energy, p->n_streams, s);
    if (rc != SFE_OK) return rc;
    p->cur ^= 1;
    p->samples += n_in;
    *n_blocks = blocks;
    return SFE_OK;
}

int sfe_dsp_corr_reset(sfe_corr_t h)
{
    Corr *p = as_corr(h);
    if (!p) return SFE_EINVAL;
    SFE_ON_DEVICE(p->device);
    SFE_HIP(hipDeviceSynchronize());
    for (int i = 0; i < 2; i++) SFE_HIP(hipMemset(p->d_hist[i], 0, p->hist_bytes()));
    SFE_HIP(hipDeviceSynchronize());
    p->cur = 0;
    p->samples = 0;
    return SFE_OK;
}

int sfe_dsp_corr_destroy(sfe_corr_t h)
{
    Corr *p = as_corr(h);
    if (!p) return SFE_OK;
    DeviceGuard g(p->device);
    (void)hipDeviceSynchronize();
    corr_free(p);
    return SFE_OK;
}

}  // extern "C"
