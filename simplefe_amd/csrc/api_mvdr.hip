// api_mvdr.hip -- the weight-solver handle behind sfe_mvdr_t, sfe_dsp_mvdr_* (include/sfe_dsp.h).  Host code only; the
// kernels are in mvdr.hip.  Here: the checks, the float64 twin of the kernel's law (sfe_dsp_mvdr_plan: the CPU fallback
// and what the host tests pin against numpy), the fallback table -- the conventional beamformer of every steering
// vector, formed in float64 and rounded once -- and the hand-over of a device matrix to a live beamformer handle.
#include <cmath>

#include "host.h"
#include "block.h"
#include "mvdr.h"
#include "beam.h"
#include "beam_view.h"

namespace sfe {
namespace {

struct Mvdr {
    static constexpr uint32_t MAGIC = 0x4d564431u;   // 'MVD1'
    uint32_t magic = MAGIC;
    int S = 0, B = 0, M = 1, wl = 0, device = 0;
    float load_rel = 0.0f, load_abs = 0.0f;
    DevBuf<float> d_steer;          // [M][B][S] (re, im)
    DevBuf<float> d_fallback;       // [M][2B][2S]
};

Mvdr *as_mvdr(void *h) { return as_handle<Mvdr>(h, "weight-solver"); }

int mvdr_check_loading(float load_rel, float load_abs)
{
    if (!std::isfinite(load_rel) || !std::isfinite(load_abs) || load_rel < 0.0f || load_abs < 0.0f) {
        set_error("mvdr: load_rel and load_abs must be finite and not negative");
        return SFE_EINVAL;
    }
    return SFE_OK;
}

int mvdr_check_steering(int S, int B, int M, const float *a)
{
    if (!a) {
        set_error("mvdr: null steering");
        return SFE_EINVAL;
    }
    for (size_t v = 0; v < (size_t)M * B; v++) {
        bool any = false;
        for (size_t i = 0; i < 2 * (size_t)S; i++) {
            const float x = a[v * 2 * S + i];
            if (!std::isfinite(x)) {
                set_error("mvdr: steering value %zu of beam %zu (band %zu) is not finite", i / 2, v % B, v / B);
                return SFE_EINVAL;
            }
            any = any || x != 0.0f;
        }
        if (!any) {
            set_error("mvdr: the steering vector of beam %zu (band %zu) is zero", v % B, v / B);
            return SFE_EINVAL;
        }
    }
    return SFE_OK;
}

int mvdr_check(int S, int B, int M, const float *steering, int wl, float load_rel, float load_abs)
{
    if (S < 1 || S > MVDR_MAX_IN) {
        set_error("mvdr: n_in = %d must be in [1, %d]", S, MVDR_MAX_IN);
        return SFE_EINVAL;
    }
    if (B < 1 || B > MVDR_MAX_BEAMS) {
        set_error("mvdr: n_beams = %d must be in [1, %d]", B, MVDR_MAX_BEAMS);
        return SFE_EINVAL;
    }
    if (M < 1 || M > MVDR_MAX_BANDS) {
        set_error("mvdr: n_bands = %d must be in [1, %d]", M, MVDR_MAX_BANDS);
        return SFE_EINVAL;
    }
    if ((long long)M * B * S > MVDR_MAX_WEIGHTS) {
        set_error("mvdr: n_bands n_beams n_in = %lld must be at most 2^20", (long long)M * B * S);
        return SFE_EINVAL;
    }
    if (wl != 0 && wl != 1) {
        set_error("mvdr: widely_linear = %d must be 0 or 1", wl);
        return SFE_EINVAL;
    }
    const int rc = mvdr_check_loading(load_rel, load_abs);
    if (rc != SFE_OK) return rc;
    return mvdr_check_steering(S, B, M, steering);
}

// The conventional beamformer W = conj(a) / |a|^2, V = 0, as the beamformer's real matrix [M][2B][2S]
std::vector<float> mvdr_fallback(int S, int B, int M, const float *a)
{
    const size_t n = 2 * (size_t)S;
    std::vector<float> R((size_t)M * 2 * B * n);
    for (size_t v = 0; v < (size_t)M * B; v++) {
        const float *av = a + v * n;
        double nrm = 0.0;
        for (size_t i = 0; i < n; i++) nrm += (double)av[i] * av[i];
        float *r0 = R.data() + 2 * v * n, *r1 = r0 + n;
        for (size_t s = 0; s < (size_t)S; s++) {
            const float wr = (float)(av[2 * s] / nrm), wi = (float)(av[2 * s + 1] / nrm);     // W = wr - j wi
            r0[2 * s] = wr;
            r0[2 * s + 1] = wi;
            r1[2 * s] = -wi;
            r1[2 * s + 1] = wr;
        }
    }
    return R;
}

bool pos_finite(double v) { return std::isfinite(v) && v > 0.0; }

// L^-T L^-1 u in place; L full n x n, lower
void chol_solve(const std::vector<double> &L, size_t n, double *z)
{
    for (size_t i = 0; i < n; i++) {
        double acc = z[i];
        for (size_t p = 0; p < i; p++) acc -= L[i * n + p] * z[p];
        z[i] = acc / L[i * n + i];
    }
    for (size_t i = n; i-- > 0;) {
        double acc = z[i];
        for (size_t p = i + 1; p < n; p++) acc -= L[p * n + i] * z[p];
        z[i] = acc / L[i * n + i];
    }
}

// The law of include/sfe_dsp.h on one problem in float64, rounded once on the way out.  G: n x n float32, only i <= j
// read; a: the band's steering [B][S]; fb: its fallback rows [2B][2S].  R, power may be null.
int mvdr_solve_host(int S, int B, int wl, double load_rel, double load_abs, const float *G, const float *a, const float *fb, float *R,
                    float *power)
{
    const size_t n = 2 * (size_t)S;
    std::vector<double> L(n * n, 0.0);
    auto up = [&](size_t i, size_t j) { return (double)(i <= j ? G[i * n + j] : G[j * n + i]); };
    for (size_t s = 0; s < (size_t)S; s++)
        for (size_t t = 0; t < (size_t)S; t++) {
            const double g00 = up(2 * s, 2 * t), g01 = up(2 * s, 2 * t + 1), g10 = up(2 * s + 1, 2 * t), g11 = up(2 * s + 1, 2 * t + 1);
            double *l0 = &L[2 * s * n + 2 * t], *l1 = l0 + n;
            if (wl) {
                l0[0] = g00, l0[1] = g01, l1[0] = g10, l1[1] = g11;
            } else {
                l0[0] = l1[1] = 0.5 * (g00 + g11);
                l1[0] = 0.5 * (g10 - g01);
                l0[1] = -l1[0];
            }
        }
    double tr = 0.0;
    for (size_t i = 0; i < n; i++) tr += L[i * n + i];
    const double lam = load_abs + load_rel * tr / (double)n;
    for (size_t i = 0; i < n; i++) L[i * n + i] += lam;
    bool ok = true;
    for (size_t k = 0; k < n && ok; k++) {
        double d = L[k * n + k];
        for (size_t p = 0; p < k; p++) d -= L[k * n + p] * L[k * n + p];
        if (!pos_finite(d)) {
            ok = false;
            break;
        }
        const double lkk = sqrt(d);
        L[k * n + k] = lkk;
        for (size_t i = k + 1; i < n; i++) {
            double v = L[i * n + k];
            for (size_t p = 0; p < k; p++) v -= L[i * n + p] * L[k * n + p];
            L[i * n + k] = v / lkk;
        }
    }
    int status = ok ? 0 : 1;
    std::vector<double> z0(n), z1(n), u0(n), u1(n);
    const float qnan = std::nanf("");
    for (size_t b = 0; b < (size_t)B; b++) {
        float *r0 = R ? R + 2 * b * n : nullptr, *r1 = R ? r0 + n : nullptr;
        bool good = ok;
        double pw = 0.0;
        if (ok) {
            for (size_t s = 0; s < (size_t)S; s++) {
                const double re = a[(b * S + s) * 2], im = a[(b * S + s) * 2 + 1];
                u0[2 * s] = re, u0[2 * s + 1] = im;
                u1[2 * s] = -im, u1[2 * s + 1] = re;
            }
            if (wl && S == 1) {     // A2 is square: R = A2^-1, the fallback's own value, and Q^-1 = A2^-1 G^ A2^-T
                if (R) memcpy(r0, fb + 2 * b * n, 2 * n * sizeof(float));
                if (power) power[b] = (float)((tr + 2.0 * lam) / (u0[0] * u0[0] + u0[1] * u0[1]));
                continue;
            }
            z0 = u0;
            chol_solve(L, n, z0.data());
            double q00 = 0.0;
            for (size_t i = 0; i < n; i++) q00 += u0[i] * z0[i];
            if (!wl) {
                good = pos_finite(q00);
                pw = 2.0 / q00;
                if (good && R)
                    for (size_t s = 0; s < (size_t)S; s++) {
                        r0[2 * s] = r1[2 * s + 1] = (float)(z0[2 * s] / q00);
                        r0[2 * s + 1] = (float)(z0[2 * s + 1] / q00);
                        r1[2 * s] = -r0[2 * s + 1];
                    }
            } else {
                z1 = u1;
                chol_solve(L, n, z1.data());
                double q01 = 0.0, q11 = 0.0;
                for (size_t i = 0; i < n; i++) q01 += u0[i] * z1[i], q11 += u1[i] * z1[i];
                const double det = q00 * q11 - q01 * q01;
                good = pos_finite(det);
                pw = (q00 + q11) / det;
                if (good && R)
                    for (size_t i = 0; i < n; i++) {
                        r0[i] = (float)((q11 * z0[i] - q01 * z1[i]) / det);
                        r1[i] = (float)((q00 * z1[i] - q01 * z0[i]) / det);
                    }
            }
        }
        if (!good) {
            if (R) memcpy(r0, fb + 2 * b * n, 2 * n * sizeof(float));
            if (ok) status = 2;
        }
        if (power) power[b] = good ? (float)pw : qnan;
    }
    return status;
}

}  // namespace
}  // namespace sfe

using namespace sfe;

extern "C" {

int sfe_dsp_mvdr_plan(int n_in, int n_beams, int n_bands, const float *steering, int widely_linear, float load_rel, float load_abs,
                      const float *gram, float *real_matrix, float *power, int *status)
{
    const int rc = mvdr_check(n_in, n_beams, n_bands, steering, widely_linear, load_rel, load_abs);
    if (rc != SFE_OK) return rc;
    if (!gram) return SFE_OK;
    const size_t n = 2 * (size_t)n_in, B = (size_t)n_beams;
    const std::vector<float> fb = mvdr_fallback(n_in, n_beams, n_bands, steering);
    for (size_t k = 0; k < (size_t)n_bands; k++) {
        const int st = mvdr_solve_host(n_in, n_beams, widely_linear, load_rel, load_abs, gram + k * n * n, steering + k * B * n,
                                       fb.data() + k * 2 * B * n, real_matrix ? real_matrix + k * 2 * B * n : nullptr,
                                       power ? power + k * B : nullptr);
        if (status) status[k] = st;
    }
    return SFE_OK;
}

int sfe_dsp_mvdr_create(const float *steering, int n_in, int n_beams, int n_bands, int widely_linear, float load_rel, float load_abs,
                        int device, sfe_mvdr_t *out)
{
    if (!out) return SFE_EINVAL;
    *out = nullptr;
    int rc = mvdr_check(n_in, n_beams, n_bands, steering, widely_linear, load_rel, load_abs);
    if (rc != SFE_OK) return rc;
    CreateScope scope(device);
    if (scope.rc != SFE_OK) return scope.rc;
    std::unique_ptr<Mvdr> p(new (std::nothrow) Mvdr);
    if (!p) return SFE_ENOMEM;
    p->S = n_in;
    p->B = n_beams;
    p->M = n_bands;
    p->wl = widely_linear;
    p->load_rel = load_rel;
    p->load_abs = load_abs;
    p->device = device;
    if ((rc = p->d_steer.upload(steering, (size_t)n_bands * n_beams * n_in * 2)) != SFE_OK ||
        (rc = p->d_fallback.upload(mvdr_fallback(n_in, n_beams, n_bands, steering))) != SFE_OK)
        return rc;
    SFE_HIP(hipDeviceSynchronize());
    *out = p.release();
    return SFE_OK;
}

int sfe_dsp_mvdr_set_steering(sfe_mvdr_t h, const float *steering)
{
    Mvdr *p = as_mvdr(h);
    if (!p) return SFE_EINVAL;
    const int rc = mvdr_check_steering(p->S, p->B, p->M, steering);
    if (rc != SFE_OK) return rc;
    const std::vector<float> fb = mvdr_fallback(p->S, p->B, p->M, steering);
    SFE_ON_DEVICE(p->device);
    // calls already enqueued read both tables: they finish with the old ones before they are replaced
    SFE_HIP(hipDeviceSynchronize());
    SFE_HIP(hipMemcpy(p->d_steer, steering, (size_t)p->M * p->B * p->S * 2 * sizeof(float), hipMemcpyHostToDevice));
    SFE_HIP(hipMemcpy(p->d_fallback, fb.data(), fb.size() * sizeof(float), hipMemcpyHostToDevice));
    SFE_HIP(hipDeviceSynchronize());
    return SFE_OK;
}

int sfe_dsp_mvdr_set_loading(sfe_mvdr_t h, float load_rel, float load_abs)
{
    Mvdr *p = as_mvdr(h);
    if (!p) return SFE_EINVAL;
    const int rc = mvdr_check_loading(load_rel, load_abs);
    if (rc != SFE_OK) return rc;
    p->load_rel = load_rel;     // a call takes the two by value when it is enqueued
    p->load_abs = load_abs;
    return SFE_OK;
}

int sfe_dsp_mvdr_process_stream(sfe_mvdr_t h, const void *d_gram, size_t n_rows, size_t in_stride, void *d_real_matrix,
                                size_t out_stride, void *d_power, size_t power_stride, void *d_status, size_t status_stride,
                                size_t *n_out, sfe_stream_t stream)
{
    static const char who[] = "mvdr_process_stream";
    Mvdr *p = stream_handle(as_mvdr(h), who, n_out);
    if (!p) return SFE_EINVAL;
    const size_t M = (size_t)p->M, B = (size_t)p->B, n2 = 2 * (size_t)p->S, gram = n2 * n2, mat = 2 * B * n2;
    if (n_rows >= ((size_t)1 << 31) / gram) {
        set_error("mvdr_process_stream: n_rows = %zu must be below 2^31 / (2 n_in)^2 = %zu per call", n_rows, ((size_t)1 << 31) / gram);
        return SFE_EINVAL;
    }
    if (n_rows == 0) return SFE_OK;
    int rc = refuse_null(who, {d_gram, d_real_matrix});
    if (rc != SFE_OK) return rc;
    if (out_stride < M * mat || (d_power && power_stride < M * B) || (d_status && status_stride < M)) {
        set_error("mvdr_process_stream: out_stride %zu < n_bands * 4 n_beams n_in = %zu, power_stride %zu < n_bands * n_beams = %zu or "
                  "status_stride %zu < n_bands = %zu",
                  out_stride, M * mat, power_stride, M * B, status_stride, M);
        return SFE_ERANGE;
    }
    if (in_stride < n_rows * gram) {
        set_error("mvdr_process_stream: in_stride %zu < n_rows * (2 n_in)^2 = %zu", in_stride, n_rows * gram);
        return SFE_EINVAL;
    }
    Span in, o[3];      // the matrix, the power, the status
    if (!solver_ranges(M, d_gram, n_rows, in_stride, gram,
                       {RowOut{d_real_matrix, out_stride, M * mat}, RowOut{d_power, power_stride, M * B}, RowOut{d_status, status_stride, M}}, &in, o))
        return refuse_2_62(who);
    hipStream_t s = (hipStream_t)stream;
    if ((rc = refuse_misaligned(who, "float32 and int32 4 B", {in, o[0], o[1], o[2]})) != SFE_OK ||
        (rc = refuse_overlap(who, in, {o[0], o[1], o[2]})) != SFE_OK)
        return rc;
    if (stream_is_capturing(s)) {       // set_steering may replace the tables a captured call would have pinned
        set_error("mvdr_process_stream: graph capture is not supported (set_steering may replace the steering table)");
        return SFE_ESTATE;
    }
    SFE_ON_DEVICE(p->device);
    const MvdrArgs a{static_cast<const float *>(d_gram), p->d_steer, p->d_fallback, static_cast<float *>(d_real_matrix),
                     static_cast<float *>(d_power), static_cast<int *>(d_status), (long long)in_stride, (long long)out_stride,
                     (long long)power_stride, (long long)status_stride, p->S, p->B, p->M, p->load_rel, p->load_abs};
    rc = launch_mvdr(a, p->wl, (long long)n_rows, s);
    if (rc != SFE_OK) return rc;
    *n_out = n_rows;
    return SFE_OK;
}

int sfe_dsp_mvdr_load_beam(sfe_beam_t beam, const float *d_real_matrix, sfe_stream_t stream)
{
    static const char who[] = "mvdr_load_beam";
    BeamView v;
    if (!beam || !beam_view(beam, &v)) {
        if (!beam) set_error("mvdr_load_beam: null beamformer handle");
        return SFE_EINVAL;
    }
    int rc = refuse_null(who, {d_real_matrix});
    if (rc != SFE_OK) return rc;
    const Span in{d_real_matrix, (size_t)v.M * 4 * v.B * v.S * sizeof(float), sizeof(float)};
    const Span table{v.frag, (size_t)v.M * beam_frag_floats(v.S, v.B) * sizeof(float), sizeof(float)};
    hipStream_t s = (hipStream_t)stream;
    if ((rc = refuse_misaligned(who, "float32 4 B", {in})) != SFE_OK || (rc = refuse_overlap(who, in, {table})) != SFE_OK) return rc;
    if (stream_is_capturing(s)) {       // sfe_dsp_beam_set_weights writes the same table from the host
        set_error("mvdr_load_beam: graph capture is not supported (set_weights writes the same weight table)");
        return SFE_ESTATE;
    }
    SFE_ON_DEVICE(v.device);
    return launch_mvdr_load_beam(d_real_matrix, v.frag, v.S, v.B, v.M, s);
}

int sfe_dsp_mvdr_destroy(sfe_mvdr_t h) { return destroy_handle(as_mvdr(h)); }

}  // extern "C"
