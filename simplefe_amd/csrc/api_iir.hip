// api_iir.hip -- the IIR-filter handle behind sfe_iir_t, sfe_dsp_iir_* (include/sfe_dsp.h).  Host code only; the kernels
// are in iir.hip.  Everything the kernels multiply by is computed here in float64 from the float32 coefficients of the
// law and rounded once: the powers of each section's transition matrix and the cascade's transition over one block.
#include <cmath>

#include "host.h"
#include "block.h"
#include "iir.h"

namespace sfe {
namespace {

struct Iir {
    static constexpr uint32_t MAGIC = 0x49495231u;   // 'IIR1'
    uint32_t magic = MAGIC;
    int S = 0, data_complex = 1, n_streams = 1, device = 0, in_u8 = 0;
    DevBuf<float> d_sec;            // [S][IIR_SEC_FLOATS]
    DevBuf<float> d_phi;            // [2][2S][2S]: the cascade's transition over one block, and over one group of blocks
    // carried (float): per stream and component the true state, the open group's partial fold and its start state
    // (iir.hip: struct IirSpan)
    CarriedPair state;
    GrowScratch table;              // the per-block and per-group states of one call
    unsigned long long blocks = 0;  // per stream since create / reset: the fold's groups are counted from there
    int nc() const { return data_complex ? 2 : 1; }
    size_t state_bytes() const { return (size_t)n_streams * nc() * 3 * 2 * S * sizeof(float); }
};

Iir *as_iir(void *h) { return as_handle<Iir>(h, "IIR-filter"); }

struct Mat2 {
    double m[4];
};
Mat2 mul2(const Mat2 &a, const Mat2 &b)
{
    return Mat2{{a.m[0] * b.m[0] + a.m[1] * b.m[2], a.m[0] * b.m[1] + a.m[1] * b.m[3], a.m[2] * b.m[0] + a.m[3] * b.m[2],
                 a.m[2] * b.m[1] + a.m[3] * b.m[3]}};
}

// The float32 coefficients of the law, (b0, b1, b2, a1, a2) per section, from scipy-layout rows; the refusals.
int iir_round(const double *sos, int S, float *coef)
{
    if (S < 1 || S > IIR_MAX_SECTIONS) {
        set_error("iir: n_sections = %d must be in [1, %d]", S, IIR_MAX_SECTIONS);
        return SFE_EINVAL;
    }
    if (!sos) {
        set_error("iir: null coefficients");
        return SFE_EINVAL;
    }
    for (int q = 0; q < S; q++) {
        const double *r = sos + 6 * q;
        for (int k = 0; k < 6; k++)
            if (!std::isfinite(r[k])) {
                set_error("iir: section %d has a non-finite coefficient", q);
                return SFE_EINVAL;
            }
        if (r[3] == 0.0) {
            set_error("iir: section %d has a0 = 0", q);
            return SFE_EINVAL;
        }
        float *c = coef + 5 * q;
        c[0] = (float)(r[0] / r[3]);
        c[1] = (float)(r[1] / r[3]);
        c[2] = (float)(r[2] / r[3]);
        c[3] = (float)(r[4] / r[3]);
        c[4] = (float)(r[5] / r[3]);
        for (int k = 0; k < 5; k++)
            if (!std::isfinite(c[k])) {
                set_error("iir: section %d has a coefficient outside float32 after the division by a0", q);
                return SFE_EINVAL;
            }
        // the stability triangle, on the values the kernel multiplies by
        const double a1 = c[3], a2 = c[4];
        if (!(std::fabs(a2) < 1.0 && std::fabs(a1) < 1.0 + a2)) {
            set_error("iir: section %d is not strictly stable in float32 (a1 = %.9g, a2 = %.9g: need |a2| < 1 and |a1| < 1 + a2)", q,
                      a1, a2);
            return SFE_EINVAL;
        }
    }
    return SFE_OK;
}

// One section's table (struct IirSec of iir.hip)
void iir_section_table(const float *c, float *t)
{
    const int R = 16;
    std::fill(t, t + IIR_SEC_FLOATS, 0.0f);
    std::copy(c, c + 5, t);
    const Mat2 A{{-(double)c[3], 1.0, -(double)c[4], 0.0}};
    Mat2 pw{{1.0, 0.0, 0.0, 1.0}};
    float *corr = t + 8 + 7 * 4;
    for (int k = 0; k < R; k++) {           // [1 0] A^k
        corr[2 * k] = (float)pw.m[0];
        corr[2 * k + 1] = (float)pw.m[1];
        pw = mul2(pw, A);
    }
    const Mat2 AR = pw;                     // A^16
    Mat2 sq = AR;
    for (int k = 0; k < 7; k++) {           // A^(16 2^k)
        for (int e = 0; e < 4; e++) t[8 + 4 * k + e] = (float)sq.m[e];
        sq = mul2(sq, sq);
    }
    float *P = t + 8 + 7 * 4 + R * 2;
    pw = Mat2{{1.0, 0.0, 0.0, 1.0}};
    for (int l = 0; l < 64; l++) {          // A^(16 l)
        for (int e = 0; e < 4; e++) P[4 * l + e] = (float)pw.m[e];
        pw = mul2(pw, AR);
    }
}

// The cascade as one linear system of 2S states (s.x, s.y of section 0, of section 1, ...): its transition over `block`
// samples of zero input, row-major, followed by the same over `group` blocks (each rounded once from float64)
std::vector<float> iir_phi(const float *coef, int S, int block, int group)
{
    const int n = 2 * S;
    std::vector<double> T((size_t)n * n, 0.0), u(n), y(n);
    std::fill(u.begin(), u.end(), 0.0);     // the section's input as a row over the states: zero for section 0
    for (int q = 0; q < S; q++) {
        const double b0 = coef[5 * q], b1 = coef[5 * q + 1], b2 = coef[5 * q + 2], a1 = coef[5 * q + 3], a2 = coef[5 * q + 4];
        for (int k = 0; k < n; k++) y[k] = b0 * u[k] + (k == 2 * q ? 1.0 : 0.0);
        for (int k = 0; k < n; k++) {
            T[(size_t)(2 * q) * n + k] = b1 * u[k] - a1 * y[k] + (k == 2 * q + 1 ? 1.0 : 0.0);
            T[(size_t)(2 * q + 1) * n + k] = b2 * u[k] - a2 * y[k];
        }
        u = y;
    }
    std::vector<double> tmp((size_t)n * n);
    auto square = [&](int times) {          // block and group are powers of two
        for (int b = times; b > 1; b >>= 1) {
            for (int i = 0; i < n; i++)
                for (int j = 0; j < n; j++) {
                    double acc = 0.0;
                    for (int k = 0; k < n; k++) acc += T[(size_t)i * n + k] * T[(size_t)k * n + j];
                    tmp[(size_t)i * n + j] = acc;
                }
            T.swap(tmp);
        }
    };
    square(block);
    std::vector<float> out(T.begin(), T.end());
    square(group);
    out.insert(out.end(), T.begin(), T.end());
    return out;
}

}  // namespace
}  // namespace sfe

using namespace sfe;

extern "C" {

int sfe_dsp_iir_plan(const double *sos, int n_sections, int *block, int *state_floats)
{
    float coef[5 * IIR_MAX_SECTIONS];
    const int rc = iir_round(sos, n_sections, coef);
    if (rc != SFE_OK) return rc;
    if (block) *block = iir_block();
    if (state_floats) *state_floats = 3 * 2 * n_sections;
    return SFE_OK;
}

int sfe_dsp_iir_create(const double *sos, int n_sections, int data_complex, int n_streams, int device, sfe_iir_t *out)
{
    if (!out) return SFE_EINVAL;
    *out = nullptr;
    float coef[5 * IIR_MAX_SECTIONS];
    int rc = iir_round(sos, n_sections, coef);
    if (rc != SFE_OK) return rc;
    if (n_streams < 1 || n_streams > 32767) {
        set_error("iir: n_streams = %d must be in [1, 32767]", n_streams);
        return SFE_EINVAL;
    }
    CreateScope scope(device);
    if (scope.rc != SFE_OK) return scope.rc;
    std::unique_ptr<Iir> p(new (std::nothrow) Iir);
    if (!p) return SFE_ENOMEM;
    p->S = n_sections;
    p->data_complex = data_complex ? 1 : 0;
    p->n_streams = n_streams;
    p->device = device;
    std::vector<float> sec((size_t)n_sections * IIR_SEC_FLOATS);
    for (int q = 0; q < n_sections; q++) iir_section_table(coef + 5 * q, sec.data() + (size_t)q * IIR_SEC_FLOATS);
    const std::vector<float> phi = iir_phi(coef, n_sections, iir_block(), iir_group());
    if ((rc = p->d_sec.upload(sec)) != SFE_OK || (rc = p->d_phi.upload(phi)) != SFE_OK || (rc = p->state.alloc_zero(p->state_bytes())) != SFE_OK)
        return rc;
    SFE_HIP(hipDeviceSynchronize());
    *out = p.release();
    return SFE_OK;
}

int sfe_dsp_iir_set_input_format(sfe_iir_t h, int fmt)
{
    Iir *p = as_iir(h);
    if (!p || (fmt != SFE_FMT_F32 && fmt != SFE_FMT_U8)) {
        set_error("iir_set_input_format: null handle or a format other than SFE_FMT_F32 / SFE_FMT_U8");
        return SFE_EINVAL;
    }
    if (fmt == SFE_FMT_U8 && !p->data_complex) {
        set_error("iir_set_input_format: SFE_FMT_U8 is (I,Q) byte pairs: not for a real handle");
        return SFE_EINVAL;
    }
    p->in_u8 = fmt == SFE_FMT_U8;
    return SFE_OK;
}

int sfe_dsp_iir_process_stream(sfe_iir_t h, const void *d_in, size_t n_in, size_t in_stride, void *d_out, size_t out_stride,
                               size_t *n_out, sfe_stream_t stream)
{
    static const char who[] = "iir_process_stream";
    Iir *p = stream_handle(as_iir(h), who, n_out);
    if (!p) return SFE_EINVAL;
    const size_t G = (size_t)iir_block();
    if (n_in % G) {
        set_error("iir_process_stream: n_in = %zu is not a multiple of the block = %zu", n_in, G);
        return SFE_EINVAL;
    }
    static const StreamNouns nouns{"n_in = ", "cf32 8 B, u8 (I,Q) pairs 2 B, float32 4 B", true, true};
    bool go;
    int rc = check_streams(who, nouns, d_in, n_in, in_stride, p->n_streams, p->in_u8 ? 2 : p->data_complex ? 8 : 4, d_out, out_stride, n_in,
                           p->n_streams, p->data_complex ? 8 : 4, &go);
    if (rc != SFE_OK || !go) return rc;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = refuse_capture(who, "sample", s)) != SFE_OK) return rc;       // counted in blocks
    SFE_ON_DEVICE(p->device);
    // the one allocation a call may make: the table of block and group states grows when a larger call than any before arrives
    // (sized for the most groups a call of nb blocks can touch, wherever it starts)
    const size_t nb = n_in / G, K = (size_t)iir_group(), need = (nb + (nb + K - 2) / K + 1) * p->n_streams * p->nc() * 2 * p->S;
    rc = p->table.reserve(need * sizeof(float));
    if (rc != SFE_OK) return rc;
    const int fmt = p->in_u8 ? 1 : p->data_complex ? 0 : 2;
    const int n2 = 2 * p->S;
    rc = launch_iir(fmt, d_in, (long long)in_stride, d_out, (long long)out_stride, p->d_sec, p->d_phi, p->d_phi + n2 * n2,
                    p->table.as<float>(), p->state.cur<float>(), p->state.next<float>(), (long long)p->blocks, (int)nb, p->S, p->n_streams,
                    s);
    if (rc != SFE_OK) return rc;
    p->state.flip();
    p->blocks += nb;
    *n_out = n_in;
    return SFE_OK;
}

int sfe_dsp_iir_reset(sfe_iir_t h)
{
    Iir *p = as_iir(h);
    if (!p) return SFE_EINVAL;
    const int rc = reset_pairs(p->device, {&p->state});
    if (rc == SFE_OK) p->blocks = 0;
    return rc;
}

int sfe_dsp_iir_destroy(sfe_iir_t h) { return destroy_handle(as_iir(h)); }

}  // extern "C"
