// api_occ.hip -- the occupancy detector's handle behind sfe_occ_t, sfe_dsp_occ_* (include/sfe_dsp.h), and the host plan.  Host
// code only; the kernel is occ.hip, the law both run is occ_law.h.
#include <cmath>

#include "host.h"
#include "block.h"
#include "occ.h"
#include "occ_law.h"

namespace sfe {
namespace {

struct Occ {
    static constexpr uint32_t MAGIC = 0x4f434331u;   // 'OCC1'
    uint32_t magic = MAGIC;
    int device = 0;
    OccParams p{};
};

Occ *as_occ(void *h) { return as_handle<Occ>(h, "occupancy detector"); }

int occ_check(int n_bins, int rank, float factor, float min_level, int gap, int min_width, int max_emissions, int shift, OccParams *p)
{
    if (n_bins < OCC_MIN_BINS || n_bins > OCC_MAX_BINS) {
        set_error("occ: n_bins = %d must be in [%d, %d]", n_bins, OCC_MIN_BINS, OCC_MAX_BINS);
        return SFE_EINVAL;
    }
    if (shift != 0 && shift != 1) {
        set_error("occ: shift = %d is neither 0 nor 1", shift);
        return SFE_EINVAL;
    }
    if (shift && (n_bins & 1)) {
        set_error("occ: n_bins = %d must be even with shift", n_bins);
        return SFE_EINVAL;
    }
    if (rank < 0 || rank >= n_bins) {
        set_error("occ: rank = %d must be in [0, n_bins = %d)", rank, n_bins);
        return SFE_EINVAL;
    }
    if (!std::isfinite(factor) || !(factor > 0.0f)) {
        set_error("occ: factor must be finite and above 0");
        return SFE_EINVAL;
    }
    if (!std::isfinite(min_level)) {
        set_error("occ: min_level is not finite");
        return SFE_EINVAL;
    }
    if (gap < 0 || gap >= n_bins) {
        set_error("occ: gap = %d must be in [0, n_bins = %d)", gap, n_bins);
        return SFE_EINVAL;
    }
    if (min_width < 1 || min_width > n_bins) {
        set_error("occ: min_width = %d must be in [1, n_bins = %d]", min_width, n_bins);
        return SFE_EINVAL;
    }
    if (max_emissions < 1 || max_emissions > OCC_MAX_EMISSIONS) {
        set_error("occ: max_emissions = %d must be in [1, %d]", max_emissions, OCC_MAX_EMISSIONS);
        return SFE_EINVAL;
    }
    *p = OccParams{n_bins, rank, gap, min_width, max_emissions, shift, factor, min_level};
    return SFE_OK;
}

}  // namespace
}  // namespace sfe

using namespace sfe;

extern "C" {

int sfe_dsp_occ_plan(int n_bins, int rank, float factor, float min_level, int gap, int min_width, int max_emissions, int shift,
                     const float *rows, size_t n_rows, sfe_occ_info *info, sfe_occ_rec *rec, uint8_t *mask)
{
    OccParams p;
    const int rc = occ_check(n_bins, rank, factor, min_level, gap, min_width, max_emissions, shift, &p);
    if (rc != SFE_OK) return rc;
    if (n_rows == 0) return SFE_OK;
    if (!rows) {
        set_error("occ: null rows");
        return SFE_EINVAL;
    }
    for (size_t i = 0; i < n_rows; i++)
        occ_plan_row(p, rows + i * (size_t)p.n, info ? info + i : nullptr, rec ? rec + i * (size_t)p.n_em : nullptr,
                     mask ? mask + i * (size_t)p.n : nullptr);
    return SFE_OK;
}

int sfe_dsp_occ_create(int n_bins, int rank, float factor, float min_level, int gap, int min_width, int max_emissions, int shift,
                       int device, sfe_occ_t *out)
{
    if (!out) return SFE_EINVAL;
    *out = nullptr;
    OccParams p;
    const int rc = occ_check(n_bins, rank, factor, min_level, gap, min_width, max_emissions, shift, &p);
    if (rc != SFE_OK) return rc;
    CreateScope scope(device);
    if (scope.rc != SFE_OK) return scope.rc;
    std::unique_ptr<Occ> h(new (std::nothrow) Occ);
    if (!h) return SFE_ENOMEM;
    h->p = p;
    h->device = device;
    *out = h.release();
    return SFE_OK;
}

int sfe_dsp_occ_process_stream(sfe_occ_t h, const float *d_in, size_t n_streams, size_t n_rows, size_t in_stride, sfe_occ_info *d_info,
                               sfe_occ_rec *d_rec, uint8_t *d_mask, size_t out_stride, size_t *n_done, sfe_stream_t stream)
{
    static const char who[] = "occ_process_stream";
    Occ *c = stream_handle(as_occ(h), who, n_done, "n_done");
    if (!c) return SFE_EINVAL;
    size_t total;
    if (__builtin_mul_overflow(n_streams, n_rows, &total) || total >= ((size_t)1 << 31)) {
        set_error("occ_process_stream: n_streams * n_rows = %zu * %zu must be below 2^31 per call", n_streams, n_rows);
        return SFE_EINVAL;
    }
    if (total == 0) return SFE_OK;
    int rc = refuse_null(who, {d_in, d_info, d_rec});
    if (rc != SFE_OK) return rc;
    if (out_stride < n_rows) {
        set_error("occ_process_stream: out_stride %zu < n_rows = %zu", out_stride, n_rows);
        return SFE_ERANGE;
    }
    const size_t N = (size_t)c->p.n, E = (size_t)c->p.n_em;
    if (n_streams > 1 && in_stride < n_rows * N) {
        set_error("occ_process_stream: in_stride %zu < n_rows * n_bins = %zu with %zu streams", in_stride, n_rows * N, n_streams);
        return SFE_EINVAL;
    }
    size_t in_b, info_b, rec_b, mask_b = 0;
    if (!span_bytes(n_streams - 1, in_stride, n_rows * N, sizeof(float), &in_b) ||
        !span_bytes(n_streams - 1, out_stride, n_rows, sizeof(sfe_occ_info), &info_b) ||
        !span_bytes(n_streams - 1, out_stride, n_rows, sizeof(sfe_occ_rec) * E, &rec_b) ||
        (d_mask && !span_bytes(n_streams - 1, out_stride, n_rows, N, &mask_b)))
        return refuse_2_62(who);
    const Span in{d_in, in_b, sizeof(float)}, info{d_info, info_b, 4}, rec{d_rec, rec_b, 4}, mask{d_mask, mask_b, 1};
    if ((rc = refuse_misaligned(who, "float32, info and records 4 B", {in, info, rec})) != SFE_OK ||
        (rc = refuse_overlap(who, in, {info, rec, mask})) != SFE_OK)
        return rc;
    if (ranges_overlap(info.p, info.bytes, rec.p, rec.bytes) || ranges_overlap(info.p, info.bytes, mask.p, mask.bytes) ||
        ranges_overlap(rec.p, rec.bytes, mask.p, mask.bytes)) {
        set_error("occ_process_stream: two output ranges overlap");
        return SFE_EINVAL;
    }
    SFE_ON_DEVICE(c->device);
    OccArgs a;
    a.in = d_in;
    a.info = d_info;
    a.rec = d_rec;
    a.mask = d_mask;
    a.in_stride = (long long)in_stride;
    a.out_stride = (long long)out_stride;
    a.n_rows = (unsigned)n_rows;
    a.p = c->p;
    rc = launch_occ(a, (unsigned)n_streams, (hipStream_t)stream);
    if (rc != SFE_OK) return rc;
    *n_done = total;
    return SFE_OK;
}

int sfe_dsp_occ_destroy(sfe_occ_t h) { return destroy_handle(as_occ(h)); }

}  // extern "C"
