// api_psd.hip -- the spectrum-estimator handle behind sfe_psd_t, sfe_dsp_psd_* (include/sfe_dsp.h).  Host code only; the
// kernels are in psd.hip.
#include <cmath>

#include "host.h"
#include "block.h"

namespace sfe {

// psd.hip
long long psd_pieces(long long j0, long long q, int A, int C, long long *rows);
int launch_psd(int logn, int u8, const void *in, long long in_stride, const v2f *hist, v2f *hist_next, const float *win, const v2f *tw,
               const float *chunk_in, float *chunk_out, const float *row_in, float *row_out, float *scratch, float *out,
               long long out_stride, long long n_in, int H, int A, int C, long long j0, float scale, int n_streams, hipStream_t st);

namespace {

struct Psd {
    static constexpr uint32_t MAGIC = 0x50534431u;   // 'PSD1'
    uint32_t magic = MAGIC;
    int N = 0, logn = 0, H = 0, A = 0, C = 0, n_streams = 1, device = 0, in_u8 = 0;
    float scale = 1.0f;
    DevBuf<float> d_win;            // [N]
    DevBuf<v2f> d_tw;               // [N]: exp(-j 2 pi q / N)
    // carried state, per stream, three pairs that flip together: N - H history samples (cf32), the open chunk's and the
    // open row's folds (float)
    CarriedPair hist, chunk, row;
    GrowScratch scratch;            // the chunk sums of one call
    unsigned long long seg = 0;     // segments per stream since create / reset
    size_t hist_bytes() const { return std::max<size_t>((size_t)n_streams * (N - H), 1) * sizeof(v2f); }
    size_t acc_bytes() const { return (size_t)n_streams * N * sizeof(float); }
};

Psd *as_psd(void *h) { return as_handle<Psd>(h, "spectrum-estimator"); }

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
    CreateScope scope(device);
    if (scope.rc != SFE_OK) return scope.rc;
    std::unique_ptr<Psd> p(new (std::nothrow) Psd);
    if (!p) return SFE_ENOMEM;
    p->N = n_fft;
    p->logn = logn;
    p->H = hop;
    p->A = n_avg;
    p->C = chunk;
    p->scale = scale;
    p->n_streams = n_streams;
    p->device = device;
    if ((rc = p->d_win.upload(window, n_fft)) != SFE_OK || (rc = p->d_tw.upload(unit_circle(n_fft, -1))) != SFE_OK ||
        (rc = p->hist.alloc_zero(p->hist_bytes())) != SFE_OK || (rc = p->chunk.alloc_zero(p->acc_bytes())) != SFE_OK ||
        (rc = p->row.alloc_zero(p->acc_bytes())) != SFE_OK)
        return rc;
    SFE_HIP(hipDeviceSynchronize());
    *out = p.release();
    return SFE_OK;
}

int sfe_dsp_psd_set_input_format(sfe_psd_t h, int fmt)
{
    return set_format(as_psd(h), "psd_set_input_format", fmt, SFE_FMT_U8, "SFE_FMT_U8", &Psd::in_u8);
}

int sfe_dsp_psd_process_stream(sfe_psd_t h, const void *d_in, size_t n_in, size_t in_stride, void *d_out, size_t out_stride,
                               size_t *n_rows, sfe_stream_t stream)
{
    static const char who[] = "psd_process_stream";
    Psd *p = stream_handle(as_psd(h), who, n_rows, "n_rows");
    if (!p) return SFE_EINVAL;
    if (n_in % (size_t)p->H) {
        set_error("psd_process_stream: n_in = %zu is not a multiple of hop = %d", n_in, p->H);
        return SFE_EINVAL;
    }
    static const StreamNouns nouns{"n_rows * n_fft = ", "cf32 8 B, u8 (I,Q) pairs 2 B, float32 rows 4 B", true, true};
    const size_t q = n_in / p->H, j0 = (size_t)(p->seg % (unsigned long long)p->A), rows = (j0 + q) / p->A;
    bool go;
    int rc = check_streams(who, nouns, d_in, n_in, in_stride, p->n_streams, p->in_u8 ? 2 : 8, d_out, out_stride, rows * p->N, p->n_streams,
                           sizeof(float), &go);
    if (rc != SFE_OK || !go) return rc;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = refuse_capture(who, "segment", s)) != SFE_OK) return rc;
    SFE_ON_DEVICE(p->device);
    // the one allocation a call may make: the scratch of chunk sums grows when a larger call than any before arrives
    // (none when a chunk is a whole row, A <= 2: the rows are written without it)
    const size_t need = (p->A + p->C - 1) / p->C > 1 ? (size_t)psd_pieces((long long)j0, (long long)q, p->A, p->C, nullptr) * p->n_streams * p->N : 0;
    rc = p->scratch.reserve(need * sizeof(float));
    if (rc != SFE_OK) return rc;
    rc = launch_psd(p->logn, p->in_u8, d_in, (long long)in_stride, p->hist.cur<v2f>(), p->hist.next<v2f>(), p->d_win, p->d_tw,
                    p->chunk.cur<float>(), p->chunk.next<float>(), p->row.cur<float>(), p->row.next<float>(), p->scratch.as<float>(),
                    static_cast<float *>(d_out), (long long)out_stride, (long long)n_in, p->H, p->A, p->C, (long long)j0, p->scale,
                    p->n_streams, s);
    if (rc != SFE_OK) return rc;
    p->hist.flip();
    p->chunk.flip();
    p->row.flip();
    p->seg += q;
    *n_rows = rows;
    return SFE_OK;
}

int sfe_dsp_psd_reset(sfe_psd_t h)
{
    Psd *p = as_psd(h);
    if (!p) return SFE_EINVAL;
    const int rc = reset_pairs(p->device, {&p->hist, &p->chunk, &p->row});
    if (rc == SFE_OK) p->seg = 0;
    return rc;
}

int sfe_dsp_psd_destroy(sfe_psd_t h) { return destroy_handle(as_psd(h)); }

}  // extern "C"
