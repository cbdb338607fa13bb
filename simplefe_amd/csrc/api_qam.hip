// api_qam.hip -- the mapper / demapper handle behind sfe_qam_t, sfe_dsp_qam_* (include/sfe_dsp.h).  Host code only; the
// kernels are in qam.hip.  Here: the checks, the tables of a shape, and sfe_dsp_qam_plan, which runs the host half of
// qam_law.h -- the header the kernels compile too -- and so is the reference of the device's bits.
#include <cmath>

#include "host.h"
#include "block.h"
#include "qam.h"
#include "qam_law.h"

namespace sfe {
namespace {

#define QAM_REFUSE(...)             \
    do {                            \
        set_error(__VA_ARGS__);     \
        return SFE_EINVAL;          \
    } while (0)

// a validated shape; perm and csi_index stay the caller's
int qam_check(int order, float amp, float scale, size_t n_sym, const uint32_t *perm, int csi_period, int csi_len, const uint32_t *csi_index,
              QamShape *sh)
{
    const int bps = qam_bps(order);
    if (!bps) QAM_REFUSE("qam: order = %d must be 2, 4, 16, 64 or 256", order);
    if (!std::isfinite(amp) || !(amp > 0.0f)) QAM_REFUSE("qam: amp must be finite and above 0");
    if (!std::isfinite(scale) || !(scale > 0.0f)) QAM_REFUSE("qam: scale must be finite and above 0");
    if (n_sym < 1 || n_sym > QAM_MAX_SYM) QAM_REFUSE("qam: n_sym = %zu must be in [1, 2^24]", n_sym);
    if (csi_period < 0 || csi_period > QAM_MAX_CSI_PERIOD) QAM_REFUSE("qam: csi_period = %d must be in [0, %d]", csi_period, QAM_MAX_CSI_PERIOD);
    if (csi_period > 0) {
        if (csi_len < 1 || csi_len > QAM_MAX_CSI_LEN) QAM_REFUSE("qam: csi_len = %d must be in [1, %d]", csi_len, QAM_MAX_CSI_LEN);
        if (!csi_index) QAM_REFUSE("qam: null csi_index with csi_period = %d", csi_period);
        for (int i = 0; i < csi_period; i++)
            if (csi_index[i] >= (uint32_t)csi_len) QAM_REFUSE("qam: csi_index[%d] = %u must be below csi_len = %d", i, csi_index[i], csi_len);
    }
    const size_t B = n_sym * (size_t)bps;
    if (perm) {
        std::vector<bool> seen(B, false);
        for (size_t t = 0; t < B; t++) {
            if (perm[t] >= B) QAM_REFUSE("qam: perm[%zu] = %u must be below n_sym * bps = %zu", t, perm[t], B);
            if (seen[perm[t]]) QAM_REFUSE("qam: perm[%zu] = %u repeats an earlier entry (perm must be a permutation)", t, perm[t]);
            seen[perm[t]] = true;
        }
    }
    sh->order = order, sh->bps = bps, sh->m = qam_axis_bits(bps);
    sh->csi_period = csi_period, sh->csi_len = csi_period > 0 ? csi_len : 0;
    sh->n_sym = n_sym, sh->scale = scale;
    qam_levels(order, amp, sh->lev);
    sh->perm = perm, sh->csi_index = csi_period > 0 ? csi_index : nullptr;
    return SFE_OK;
}

struct Qam {
    static constexpr uint32_t MAGIC = 0x51414d31u;   // 'QAM1'
    uint32_t magic = MAGIC;
    int device = 0;
    QamShape sh;                // never changes after create; its two pointers are null (the tables are below)
    bool has_perm = false;
    DevBuf<uint32_t> d_perm, d_csi_index;
    size_t B() const { return sh.n_sym * (size_t)sh.bps; }
    size_t row_bytes() const { return (B() + 7) / 8; }
};

Qam *as_qam(void *h) { return as_handle<Qam>(h, "mapper"); }

// what the two calls share behind their checks
int qam_args(const Qam *p, const char *who, size_t n_rows, QamArgs *a)
{
    const unsigned tiles = qam_tiles(p->sh.n_sym);
    if ((unsigned long long)tiles * n_rows >= (1ull << 31)) {
        set_error("%s: the call's workgroups (%u symbols of a row each) must number below 2^31", who, QAM_TILE);
        return SFE_EINVAL;
    }
    *a = QamArgs{};
    a->perm = p->has_perm ? p->d_perm.p : nullptr;
    a->csi_index = p->d_csi_index;
    a->n_sym = (unsigned)p->sh.n_sym, a->tiles = tiles, a->n_wg = (unsigned)(tiles * n_rows);
    a->csi_period = (unsigned)p->sh.csi_period;
    a->scale = p->sh.scale;
    for (int w = 0; w < QAM_MAX_WORDS; w++) a->lev[w] = p->sh.lev[w];
    return SFE_OK;
}

}  // namespace
}  // namespace sfe

using namespace sfe;

extern "C" {

int sfe_dsp_qam_plan(int order, float amp, float scale, size_t n_sym, const uint32_t *perm, int csi_period, int csi_len,
                     const uint32_t *csi_index, int direction, const void *in, size_t in_stride, const void *csi, size_t csi_stride,
                     size_t n_rows, void *out, size_t out_stride, int *bps, size_t *row_bytes)
{
    if (bps) *bps = 0;
    if (row_bytes) *row_bytes = 0;
    QamShape s;
    int rc = qam_check(order, amp, scale, n_sym, perm, csi_period, csi_len, csi_index, &s);
    if (rc != SFE_OK) return rc;
    const size_t B = s.n_sym * (size_t)s.bps, nbytes = (B + 7) / 8;
    if (bps) *bps = s.bps;
    if (row_bytes) *row_bytes = nbytes;
    if (direction != SFE_QAM_MAP && direction != SFE_QAM_DEMAP) QAM_REFUSE("qam: direction = %d must be SFE_QAM_MAP (0) or SFE_QAM_DEMAP (1)", direction);
    if (!in || n_rows == 0) return SFE_OK;
    if (!out) QAM_REFUSE("qam: null output with rows to run");
    const bool demap = direction == SFE_QAM_DEMAP, with_csi = demap && s.csi_period > 0;
    if (demap && (csi != nullptr) != with_csi) QAM_REFUSE("qam: csi is required exactly when csi_period > 0");
    const size_t in_row = demap ? s.n_sym : nbytes, out_row = demap ? B : s.n_sym;
    if (in_stride < in_row || out_stride < out_row || (with_csi && csi_stride < (size_t)s.csi_len)) {
        set_error("qam: in_stride %zu < the row's %zu, out_stride %zu < the row's %zu, or csi_stride %zu < csi_len = %d", in_stride, in_row, out_stride,
                  out_row, csi_stride, s.csi_len);
        return SFE_ERANGE;
    }
    const unsigned char *pi = static_cast<const unsigned char *>(in), *pc = static_cast<const unsigned char *>(csi);
    unsigned char *po = static_cast<unsigned char *>(out);
    for (size_t r = 0; r < n_rows; r++) {
        if (demap) qam_demap_row_host(s, pi + 8 * r * in_stride, with_csi ? pc + 8 * r * csi_stride : nullptr, po + 4 * r * out_stride);
        else qam_map_row_host(s, pi + r * in_stride, po + 8 * r * out_stride);
    }
    return SFE_OK;
}

int sfe_dsp_qam_create(int order, float amp, float scale, size_t n_sym, const uint32_t *perm, int csi_period, int csi_len,
                       const uint32_t *csi_index, int device, sfe_qam_t *out)
{
    if (!out) return SFE_EINVAL;
    *out = nullptr;
    std::unique_ptr<Qam> p(new (std::nothrow) Qam);
    if (!p) return SFE_ENOMEM;
    int rc = qam_check(order, amp, scale, n_sym, perm, csi_period, csi_len, csi_index, &p->sh);
    if (rc != SFE_OK) return rc;
    p->sh.perm = nullptr, p->sh.csi_index = nullptr;
    CreateScope scope(device);
    if (scope.rc != SFE_OK) return scope.rc;
    p->device = device;
    p->has_perm = perm != nullptr;
    if (perm && (rc = p->d_perm.upload(perm, p->B())) != SFE_OK) return rc;
    if (csi_period > 0 && (rc = p->d_csi_index.upload(csi_index, (size_t)csi_period)) != SFE_OK) return rc;
    *out = p.release();
    return SFE_OK;
}

int sfe_dsp_qam_map_stream(sfe_qam_t h, const void *d_bytes, size_t in_stride, size_t n_rows, void *d_sym, size_t out_stride, size_t *n_out,
                           sfe_stream_t stream)
{
    static const char who[] = "qam_map_stream";
    Qam *p = stream_handle(as_qam(h), who, n_out);
    if (!p) return SFE_EINVAL;
    static const TypedRowNouns nouns{"n_rows", "coded bytes of a row", "csi_stride", "(no csi)", "cf32 of a row",
                                     "cf32 output 8 B; coded bytes need none"};
    bool go;
    int rc = check_typed_rows(who, nouns, n_rows, d_bytes, in_stride, p->row_bytes(), 1, nullptr, 0, 0, 8, d_sym, out_stride, p->sh.n_sym, 8, &go);
    if (rc != SFE_OK || !go) return rc;
    QamArgs a;
    if ((rc = qam_args(p, who, n_rows, &a)) != SFE_OK) return rc;
    SFE_ON_DEVICE(p->device);
    a.in = d_bytes, a.out = d_sym;
    a.in_stride = (long long)in_stride, a.out_stride = (long long)out_stride;
    if ((rc = launch_qam_map(p->sh.bps, a, (hipStream_t)stream)) != SFE_OK) return rc;
    *n_out = n_rows;
    return SFE_OK;
}

int sfe_dsp_qam_demap_stream(sfe_qam_t h, const void *d_sym, size_t in_stride, const void *d_csi, size_t csi_stride, size_t n_rows, void *d_soft,
                             size_t out_stride, size_t *n_out, sfe_stream_t stream)
{
    static const char who[] = "qam_demap_stream";
    Qam *p = stream_handle(as_qam(h), who, n_out);
    if (!p) return SFE_EINVAL;
    static const TypedRowNouns nouns{"n_rows", "cf32 of a row", "csi_stride", "cf32 of a csi row", "floats of a row", "cf32 8 B, float32 4 B"};
    const bool with_csi = p->sh.csi_period > 0;
    if (n_rows > 0 && n_rows < ((size_t)1 << 31)) {
        if (with_csi && !d_csi) return refuse_null(who, {d_csi});
        if (!with_csi && d_csi) {
            set_error("%s: d_csi given to a handle without channel weighting (csi_period = 0)", who);
            return SFE_EINVAL;
        }
    }
    bool go;
    int rc = check_typed_rows(who, nouns, n_rows, d_sym, in_stride, p->sh.n_sym, 8, with_csi ? d_csi : nullptr, csi_stride, (size_t)p->sh.csi_len, 8,
                              d_soft, out_stride, p->B(), 4, &go);
    if (rc != SFE_OK || !go) return rc;
    QamArgs a;
    if ((rc = qam_args(p, who, n_rows, &a)) != SFE_OK) return rc;
    SFE_ON_DEVICE(p->device);
    a.in = d_sym, a.out = d_soft, a.csi = static_cast<const v2f *>(d_csi);
    a.in_stride = (long long)in_stride, a.out_stride = (long long)out_stride, a.csi_stride = (long long)csi_stride;
    if ((rc = launch_qam_demap(p->sh.bps, a, (hipStream_t)stream)) != SFE_OK) return rc;
    *n_out = n_rows;
    return SFE_OK;
}

int sfe_dsp_qam_destroy(sfe_qam_t h) { return destroy_handle(as_qam(h)); }

}  // extern "C"
