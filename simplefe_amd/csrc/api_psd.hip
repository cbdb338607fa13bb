// api_psd.hip -- the spectrum-estimator handle behind sfe_psd_t, sfe_dsp_psd_* (include/sfe_dsp.h).  Host code only; the
// kernels are in psd.hip.
#include <cmath>

#include "host.h"

namespace sfe {

// psd.hip
long long psd_pieces(long long j0, long long q, int A, int C, long long *rows);
int launch_psd(int logn, int u8, const void *in, long long in_stride, const v2f *hist, v2f *hist_next, const float *win, const v2f *tw,
               const float *chunk_in, float *chunk_out, const float *row_in, float *row_out, float *scratch, float *out,
               long long out_stride, long long n_in, int H, int A, int C, long long j0, float scale, int n_streams, hipStream_t st);

namespace {

struct Psd {
    uint32_t magic = 0x50534431u;   // 'PSD1'
    int N = 0, logn = 0, H = 0, A = 0, C = 0, n_streams = 1, device = 0, in_u8 = 0;
    float scale = 1.0f;
    float *d_win = nullptr;         // [N]
    v2f *d_tw = nullptr;            // [N]: exp(-j 2 pi q / N)
    // carried state, each a pair (the current one and the next call's): N - H history samples, the open chunk's and the
    // open row's folds, per stream
    v2f *d_hist[2] = {nullptr, nullptr};
    float *d_chunk[2] = {nullptr, nullptr};
    float *d_row[2] = {nullptr, nullptr};
    int cur = 0;
    float *d_scratch = nullptr;     // the chunk sums of one call; grows with the largest call seen
    size_t scratch_floats = 0;
    unsigned long long seg = 0;     // segments per stream since create / reset
    size_t hist_bytes() const { return std::max<size_t>((size_t)n_streams * (N - H), 1) * sizeof(v2f); }
    size_t acc_bytes() const { return (size_t)n_streams * N * sizeof(float); }
};

Psd *as_psd(void *h)
{
    Psd *p = static_cast<Psd *>(h);
    if (p && p->magic != 0x50534431u) {
        set_error("not a live spectrum-estimator handle");
        return nullptr;
    }
    return p;
}

void psd_free(Psd *p)
{
    if (!p) return;
    if (p->d_win) (void)hipFree(p->d_win);
    if (p->d_tw) (void)hipFree(p->d_tw);
    if (p->d_scratch) (void)hipFree(p->d_scratch);
    for (int i = 0; i < 2; i++) {
        if (p->d_hist[i]) (void)hipFree(p->d_hist[i]);
        if (p->d_chunk[i]) (void)hipFree(p->d_chunk[i]);
        if (p->d_row[i]) (void)hipFree(p->d_row[i]);
    }
    p->magic = 0;
    delete p;
}

int psd_check_shape(int N, int H, int A, int *logn, int *chunk)
{
    int lg = 0;
    while (lg < 30 && (1 << lg) < N) lg++;
    if (N < 256 || N > 4096 || (1 << lg) != N) {
        set_error("psd: n_fft = %d must be a power of two in [256, 4096]", N);
        return SFE_EINVAL;
    }
    if (H < 1 || H > N) {
        set_error("psd: hop = %d must be in [1, n_fft = %d]", H, N);
        return SFE_EINVAL;
    }
    if (A < 1 || A > (1 << 24)) {
        set_error("psd: n_avg = %d must be in [1, 2^24]", A);
        return SFE_EINVAL;
    }
    int C = 1;
    while ((long long)C * C < A) C *= 2;
    if (logn) *logn = lg;
    if (chunk) *chunk = C;
    return SFE_OK;
}

}  // namespace
}  // namespace sfe

using namespace sfe;

extern "C" {

int sfe_dsp_psd_plan(int n_fft, int hop, int n_avg, int *chunk, int *history)
{
    int C = 0;
    const int rc = psd_check_shape(n_fft, hop, n_avg, nullptr, &C);
    if (rc != SFE_OK) return rc;
    if (chunk) *chunk = C;
    if (history) *history = n_fft - hop;
    return SFE_OK;
}

int sfe_dsp_psd_create(const float *window, int n_fft, int hop, int n_avg, float scale, int n_streams, int device, sfe_psd_t *out)
{
    if (!out) return SFE_EINVAL;
    *out = nullptr;
    int logn = 0, chunk = 0;
    int rc = psd_check_shape(n_fft, hop, n_avg, &logn, &chunk);
    if (rc != SFE_OK) return rc;
    if (!window || n_streams < 1 || !std::isfinite(scale)) {
        set_error("psd_create: need a window, a finite scale and n_streams >= 1");
        return SFE_EINVAL;
    }
    int prev_dev = -1;
    (void)hipGetDevice(&prev_dev);
    rc = use_device(device);
    if (rc != SFE_OK) return rc;
    struct Restore { int d; ~Restore() { if (d >= 0) (void)hipSetDevice(d); } } restore__{prev_dev};
    Psd *p = new (std::nothrow) Psd;
    if (!p) return SFE_ENOMEM;
    p->N = n_fft;
    p->logn = logn;
    p->H = hop;
    p->A = n_avg;
    p->C = chunk;
    p->scale = scale;
    p->n_streams = n_streams;
    p->device = device;
    auto fail = [&](int code) { psd_free(p); return code; };
#define TRY(call) do { hipError_t e__ = (call); if (e__ != hipSuccess) return fail(hip_fail(e__, #call)); } while (0)
    std::vector<v2f> tw(n_fft);
    for (int q = 0; q < n_fft; q++) {
        const double a = 2.0 * M_PI * q / n_fft;
        tw[q] = v2f{(float)cos(a), (float)-sin(a)};
        if (q % (n_fft / 4) == 0) {         // the quarter turns exactly
            static const float cq[4] = {1.0f, 0.0f, -1.0f, 0.0f}, sq[4] = {0.0f, -1.0f, 0.0f, 1.0f};
            tw[q] = v2f{cq[q / (n_fft / 4)], sq[q / (n_fft / 4)]};
        }
    }
    TRY(hipMalloc(&p->d_win, (size_t)n_fft * sizeof(float)));
    TRY(hipMemcpy(p->d_win, window, (size_t)n_fft * sizeof(float), hipMemcpyHostToDevice));
    TRY(hipMalloc(&p->d_tw, tw.size() * sizeof(v2f)));
    TRY(hipMemcpy(p->d_tw, tw.data(), tw.size() * sizeof(v2f), hipMemcpyHostToDevice));
    for (int i = 0; i < 2; i++) {
        TRY(hipMalloc(&p->d_hist[i], p->hist_bytes()));
        TRY(hipMemset(p->d_hist[i], 0, p->hist_bytes()));
        TRY(hipMalloc(&p->d_chunk[i], p->acc_bytes()));
        TRY(hipMemset(p->d_chunk[i], 0, p->acc_bytes()));
        TRY(hipMalloc(&p->d_row[i], p->acc_bytes()));
        TRY(hipMemset(p->d_row[i], 0, p->acc_bytes()));
    }
    TRY(hipDeviceSynchronize());
#undef TRY
    *out = p;
    return SFE_OK;
}

int sfe_dsp_psd_set_input_format(sfe_psd_t h, int fmt)
{
    Psd *p = as_psd(h);
    if (!p || (fmt != SFE_FMT_F32 && fmt != SFE_FMT_U8)) {
        set_error("psd_set_input_format: null handle or a format other than SFE_FMT_F32 / SFE_FMT_U8");
        return SFE_EINVAL;
    }
    p->in_u8 = fmt == SFE_FMT_U8;
    return SFE_OK;
}

int sfe_dsp_psd_process_stream(sfe_psd_t h, const void *d_in, size_t n_in, size_t in_stride, void *d_out, size_t out_stride,
                               size_t *n_rows, sfe_stream_t stream)
{
    Psd *p = as_psd(h);
    if (n_rows) *n_rows = 0;
    if (!p || !n_rows) {
        set_error("psd_process_stream: null handle or n_rows");
        return SFE_EINVAL;
    }
    if (n_in % (size_t)p->H) {
        set_error("psd_process_stream: n_in = %zu is not a multiple of hop = %d", n_in, p->H);
        return SFE_EINVAL;
    }
    if (n_in >= ((size_t)1 << 31)) {
        set_error("psd_process_stream: n_in = %zu must be below 2^31", n_in);
        return SFE_EINVAL;
    }
    if (n_in == 0) return SFE_OK;
    const size_t q = n_in / p->H, j0 = (size_t)(p->seg % (unsigned long long)p->A), rows = (j0 + q) / p->A;
    if (!d_in || !d_out) {
        set_error("psd_process_stream: null buffer");
        return SFE_EINVAL;
    }
    if (out_stride < rows * p->N) {
        set_error("psd_process_stream: out_stride %zu < n_rows * n_fft = %zu", out_stride, rows * p->N);
        return SFE_ERANGE;
    }
    if (p->n_streams > 1 && in_stride < n_in) {
        set_error("psd_process_stream: in_stride %zu < n_in %zu with %d streams", in_stride, n_in, p->n_streams);
        return SFE_EINVAL;
    }
    const size_t isz = p->in_u8 ? 2 : 8;
    if ((reinterpret_cast<uintptr_t>(d_in) & (isz - 1)) || (reinterpret_cast<uintptr_t>(d_out) & 3)) {
        set_error("psd_process_stream: buffers must be aligned to their element (cf32 8 B, u8 (I,Q) pairs 2 B, float32 rows 4 B)");
        return SFE_EINVAL;
    }
    const size_t in_b = ((size_t)(p->n_streams - 1) * in_stride + n_in) * isz;
    const size_t out_b = rows ? ((size_t)(p->n_streams - 1) * out_stride + rows * p->N) * sizeof(float) : 0;
    if (out_b && ranges_overlap(d_in, in_b, d_out, out_b)) {
        set_error("psd_process_stream: input and output ranges overlap (in-place operation is not supported)");
        return SFE_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    if (stream_is_capturing(s)) {
        // the segment counter and the buffer pairs of the carried state advance on the host
        set_error("psd_process_stream: graph capture is not supported (the segment counter lives on the host)");
        return SFE_ESTATE;
    }
    SFE_ON_DEVICE(p->device);
    // the one allocation a call may make: the scratch of chunk sums grows when a larger call than any before arrives
    // (none when a chunk is a whole row, A <= 2: the rows are written without it)
    const size_t need = (p->A + p->C - 1) / p->C > 1 ? (size_t)psd_pieces((long long)j0, (long long)q, p->A, p->C, nullptr) * p->n_streams * p->N : 0;
    if (need > p->scratch_floats) {
        SFE_HIP(hipDeviceSynchronize());
        if (p->d_scratch) (void)hipFree(p->d_scratch);
        p->d_scratch = nullptr;
        p->scratch_floats = 0;
        SFE_HIP(hipMalloc(&p->d_scratch, need * sizeof(float)));
        p->scratch_floats = need;
    }
    const int c = p->cur;
    const int rc = launch_psd(p->logn, p->in_u8, d_in, (long long)in_stride, p->d_hist[c], p->d_hist[c ^ 1], p->d_win, p->d_tw,
                              p->d_chunk[c], p->d_chunk[c ^ 1], p->d_row[c], p->d_row[c ^ 1], p->d_scratch, static_cast<float *>(d_out),
                              (long long)out_stride, (long long)n_in, p->H, p->A, p->C, (long long)j0, p->scale, p->n_streams, s);
    if (rc != SFE_OK) return rc;
    p->cur ^= 1;
    p->seg += q;
    *n_rows = rows;
    return SFE_OK;
}

int sfe_dsp_psd_reset(sfe_psd_t h)
{
    Psd *p = as_psd(h);
    if (!p) return SFE_EINVAL;
    SFE_ON_DEVICE(p->device);
    SFE_HIP(hipDeviceSynchronize());
    for (int i = 0; i < 2; i++) {
        SFE_HIP(hipMemset(p->d_hist[i], 0, p->hist_bytes()));
        SFE_HIP(hipMemset(p->d_chunk[i], 0, p->acc_bytes()));
        SFE_HIP(hipMemset(p->d_row[i], 0, p->acc_bytes()));
    }
    SFE_HIP(hipDeviceSynchronize());
    p->cur = 0;
    p->seg = 0;
    return SFE_OK;
}

int sfe_dsp_psd_destroy(sfe_psd_t h)
{
    Psd *p = as_psd(h);
    if (!p) return SFE_OK;
    DeviceGuard g(p->device);
    (void)hipDeviceSynchronize();
    psd_free(p);
    return SFE_OK;
}

}  // extern "C"
