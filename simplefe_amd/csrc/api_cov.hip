// api_cov.hip -- the covariance-estimator handle behind sfe_cov_t, sfe_dsp_cov_* (include/sfe_dsp.h).  Host code only;
// the kernels are in cov.hip.
#include <cmath>

#include "host.h"
#include "block.h"
#include "cov.h"

namespace sfe {
namespace {

struct Cov {
    static constexpr uint32_t MAGIC = 0x434f5631u;   // 'COV1'
    uint32_t magic = MAGIC;
    int S = 0, M = 1, A = 0, AC = 0, C = 0, device = 0, in_u8 = 0;     // AC = A / COV_T chunks per row
    float scale = 1.0f;
    // carried state, per band, two pairs that flip together: the open group's and the open row's folds, in the
    // kernels' fragment order (cov.h)
    CarriedPair group, row;
    GrowScratch scratch;            // the group sums of one call
    unsigned long long chunks = 0;  // chunks per band since create / reset
    size_t acc_bytes() const { return (size_t)M * cov_frag_floats(S) * sizeof(float); }
};

Cov *as_cov(void *h) { return as_handle<Cov>(h, "covariance-estimator"); }

int cov_check_shape(int S, int M, int A, int *group)
{
    if (S < 1 || S > COV_MAX_IN) {
        set_error("cov: n_in_streams = %d must be in [1, %d]", S, COV_MAX_IN);
        return SFE_EINVAL;
    }
    if (M < 1 || M > COV_MAX_BANDS) {
        set_error("cov: n_bands = %d must be in [1, %d]", M, COV_MAX_BANDS);
        return SFE_EINVAL;
    }
    if (A < COV_T || A > COV_MAX_AVG || A % COV_T) {
        set_error("cov: n_avg = %d must be a positive multiple of %d, at most 2^24", A, COV_T);
        return SFE_EINVAL;
    }
    int C = 1;
    while ((long long)C * C < A / COV_T) C *= 2;
    if (group) *group = C;
    return SFE_OK;
}

}  // namespace
}  // namespace sfe

using namespace sfe;

extern "C" {

int sfe_dsp_cov_plan(int n_in_streams, int n_bands, int n_avg, int *chunk, int *group)
{
    int C = 0;
    const int rc = cov_check_shape(n_in_streams, n_bands, n_avg, &C);
    if (rc != SFE_OK) return rc;
    if (chunk) *chunk = COV_T;
    if (group) *group = C;
    return SFE_OK;
}

int sfe_dsp_cov_create(int n_in_streams, int n_bands, int n_avg, float scale, int device, sfe_cov_t *out)
{
    if (!out) return SFE_EINVAL;
    *out = nullptr;
    int C = 0;
    int rc = cov_check_shape(n_in_streams, n_bands, n_avg, &C);
    if (rc != SFE_OK) return rc;
    if (!std::isfinite(scale)) {
        set_error("cov: scale must be finite");
        return SFE_EINVAL;
    }
    CreateScope scope(device);
    if (scope.rc != SFE_OK) return scope.rc;
    std::unique_ptr<Cov> p(new (std::nothrow) Cov);
    if (!p) return SFE_ENOMEM;
    p->S = n_in_streams;
    p->M = n_bands;
    p->A = n_avg;
    p->AC = n_avg / COV_T;
    p->C = C;
    p->scale = scale;
    p->device = device;
    if ((rc = p->group.alloc_zero(p->acc_bytes())) != SFE_OK || (rc = p->row.alloc_zero(p->acc_bytes())) != SFE_OK) return rc;
    SFE_HIP(hipDeviceSynchronize());
    *out = p.release();
    return SFE_OK;
}

int sfe_dsp_cov_set_input_format(sfe_cov_t h, int fmt)
{
    return set_format(as_cov(h), "cov_set_input_format", fmt, SFE_FMT_U8, "SFE_FMT_U8", &Cov::in_u8);
}

int sfe_dsp_cov_process_stream(sfe_cov_t h, const void *d_in, size_t n_in, size_t in_stride, void *d_out, size_t out_stride,
                               size_t *n_rows, sfe_stream_t stream)
{
    static const char who[] = "cov_process_stream";
    Cov *p = stream_handle(as_cov(h), who, n_rows, "n_rows");
    if (!p) return SFE_EINVAL;
    if (n_in % (size_t)COV_T) {
        set_error("cov_process_stream: n_in = %zu is not a multiple of the chunk = %d", n_in, COV_T);
        return SFE_EINVAL;
    }
    static const StreamNouns nouns{"n_rows * (2 n_in_streams)^2 = ", "cf32 8 B, u8 (I,Q) pairs 2 B, float32 rows 4 B", true, false};
    const size_t q = n_in / COV_T, j0 = (size_t)(p->chunks % (unsigned long long)p->AC), rows = (j0 + q) / p->AC;
    const size_t n2 = 2 * (size_t)p->S, gram = n2 * n2;
    bool go;
    int rc = check_streams(who, nouns, d_in, n_in, in_stride, (size_t)p->S * p->M, p->in_u8 ? 2 : 8, d_out, out_stride, rows * gram, p->M,
                           sizeof(float), &go);
    if (rc != SFE_OK || !go) return rc;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = refuse_capture(who, "instant", s)) != SFE_OK) return rc;
    SFE_ON_DEVICE(p->device);
    // the one allocation a call may make: the scratch of group sums grows when a larger call than any before arrives
    // (none when a chunk is a whole row, A = T: the rows are written without it)
    const size_t need = p->AC > 1 ? (size_t)cov_pieces((long long)j0, (long long)q, p->AC, p->C, nullptr) * p->M * cov_frag_floats(p->S) : 0;
    rc = p->scratch.reserve(need * sizeof(float));
    if (rc != SFE_OK) return rc;
    rc = launch_cov(p->in_u8, d_in, (long long)in_stride, p->group.cur<float>(), p->group.next<float>(), p->row.cur<float>(),
                    p->row.next<float>(), p->scratch.as<float>(), static_cast<float *>(d_out), (long long)out_stride, (long long)n_in,
                    p->S, p->M, p->AC, p->C, (long long)j0, p->scale, s);
    if (rc != SFE_OK) return rc;
    p->group.flip();
    p->row.flip();
    p->chunks += q;
    *n_rows = rows;
    return SFE_OK;
}

int sfe_dsp_cov_reset(sfe_cov_t h)
{
    Cov *p = as_cov(h);
    if (!p) return SFE_EINVAL;
    const int rc = reset_pairs(p->device, {&p->group, &p->row});
    if (rc == SFE_OK) p->chunks = 0;
    return rc;
}

int sfe_dsp_cov_destroy(sfe_cov_t h) { return destroy_handle(as_cov(h)); }

}  // extern "C"
