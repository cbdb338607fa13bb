// api_eig.hip -- the eigen-solver handle behind sfe_eig_t, sfe_dsp_eig_* (include/sfe_dsp.h).  Host code only; the kernel
// is in eig.hip.  Here: the checks and the float64 twin of the kernel's law (sfe_dsp_eig_plan: the CPU fallback and what
// the host tests pin against numpy), which runs the same Jacobi method -- eig.h's pair order, rotation and block update --
// real for the widely-linear mode, complex for the linear one -- in double, with a threshold to match.
#include <cfloat>
#include <cmath>

#include "host.h"
#include "block.h"
#include "eig.h"

namespace sfe {
namespace {

struct Eig {
    static constexpr uint32_t MAGIC = 0x45494731u;   // 'EIG1'
    uint32_t magic = MAGIC;
    int S = 0, B = 0, E = 0, M = 1, wl = 0, D = 0, device = 0;
    DevBuf<float> d_steer;          // [M][B][S] (re, im); nothing with B = 0
};

Eig *as_eig(void *h) { return as_handle<Eig>(h, "eigen-solver"); }

int eig_check_signal_dim(int S, int wl, int D)
{
    if (D < 0 || D >= 2 * S) {
        set_error("eig: signal_dim = %d must be in [0, 2 n_in - 1 = %d]", D, 2 * S - 1);
        return SFE_EINVAL;
    }
    if (!wl && (D & 1)) {
        set_error("eig: signal_dim = %d must be even in the linear mode (a source takes two real dimensions)", D);
        return SFE_EINVAL;
    }
    return SFE_OK;
}

int eig_check_steering(int S, int B, int M, const float *a)
{
    if (B == 0) return SFE_OK;
    if (!a) {
        set_error("eig: null steering");
        return SFE_EINVAL;
    }
    for (size_t v = 0; v < (size_t)M * B; v++) {
        bool any = false;
        for (size_t i = 0; i < 2 * (size_t)S; i++) {
            const float x = a[v * 2 * S + i];
            if (!std::isfinite(x)) {
                set_error("eig: steering value %zu of beam %zu (band %zu) is not finite", i / 2, v % B, v / B);
                return SFE_EINVAL;
            }
            any = any || x != 0.0f;
        }
        if (!any) {
            set_error("eig: the steering vector of beam %zu (band %zu) is zero", v % B, v / B);
            return SFE_EINVAL;
        }
    }
    return SFE_OK;
}

int eig_check(int S, int B, int E, int M, const float *steering, int wl, int D)
{
    if (S < 1 || S > EIG_MAX_IN) {
        set_error("eig: n_in = %d must be in [1, %d]", S, EIG_MAX_IN);
        return SFE_EINVAL;
    }
    if (B < 0 || B > EIG_MAX_BEAMS) {
        set_error("eig: n_beams = %d must be in [0, %d]", B, EIG_MAX_BEAMS);
        return SFE_EINVAL;
    }
    if (E < 0 || E > S) {
        set_error("eig: n_vec = %d must be in [0, n_in = %d]", E, S);
        return SFE_EINVAL;
    }
    if (M < 1 || M > EIG_MAX_BANDS) {
        set_error("eig: n_bands = %d must be in [1, %d]", M, EIG_MAX_BANDS);
        return SFE_EINVAL;
    }
    const long long most = std::max(std::max(B, E), 1);
    if ((long long)M * most * S > EIG_MAX_WEIGHTS) {
        set_error("eig: n_bands max(n_beams, n_vec, 1) n_in = %lld must be at most 2^20", (long long)M * most * S);
        return SFE_EINVAL;
    }
    if (wl != 0 && wl != 1) {
        set_error("eig: widely_linear = %d must be 0 or 1", wl);
        return SFE_EINVAL;
    }
    const int rc = eig_check_signal_dim(S, wl, D);
    if (rc != SFE_OK) return rc;
    return eig_check_steering(S, B, M, steering);
}

// G^ = V diag(d) V^T by the cyclic Jacobi method of eig.h: A is n x n, symmetric, finite, and becomes diagonal; Vt, n x n,
// gets an eigenvector per row.  `scale` is what the threshold is relative to.  False at the sweep limit.
template <class T>
bool jacobi(std::vector<T> &A, std::vector<T> &Vt, int n, T scale, int tol_exp)
{
    const int h = n / 2;
    std::fill(Vt.begin(), Vt.end(), T(0));
    for (int i = 0; i < n; i++) Vt[(size_t)i * n + i] = T(1);
    const T thr = std::ldexp(scale, tol_exp);
    std::vector<T> c(h), s(h);
    std::vector<int> p(h), q(h);
    for (int sweep = 0; sweep < EIG_MAX_SWEEPS; sweep++) {
        bool big = false;
        for (int r = 0; r < n - 1; r++) {
            for (int a = 0; a < h; a++) {
                eig_pair(n, r, a, &p[a], &q[a]);
                const T app = A[(size_t)p[a] * n + p[a]], apq = A[(size_t)p[a] * n + q[a]], aqq = A[(size_t)q[a] * n + q[a]];
                T t;
                eig_rotation(app, apq, aqq, &c[a], &s[a], &t);
                if (apq != T(0)) {
                    A[(size_t)p[a] * n + p[a]] = eig_fma(-t, apq, app);
                    A[(size_t)q[a] * n + q[a]] = eig_fma(t, apq, aqq);
                    A[(size_t)p[a] * n + q[a]] = A[(size_t)q[a] * n + p[a]] = T(0);
                    big = big || std::fabs(apq) > thr;
                }
            }
            for (int a = 0; a < h; a++) {
                T *Ap = &A[(size_t)p[a] * n], *Aq = &A[(size_t)q[a] * n];
                for (int b = 0; b < h; b++)
                    if (a != b) eig_block(a > b, c[a], s[a], c[b], s[b], &Ap[p[b]], &Ap[q[b]], &Aq[p[b]], &Aq[q[b]]);
                for (int j = 0; j < n; j++) eig_rot2(c[a], s[a], &Vt[(size_t)p[a] * n + j], &Vt[(size_t)q[a] * n + j]);
            }
        }
        if (!big) return true;
    }
    return false;
}

// The linear mode's form: Z = V diag(d) V^H, Z m x m Hermitian as (re, im) pairs, by the complex rotations of eig.h; Vt,
// m rows of ldv scalars, gets a complex eigenvector w per row as u(w) (S components: a phantom index has none).
template <class T>
bool jacobi_c(std::vector<T> &Z, std::vector<T> &Vt, int m, int S, T scale, int tol_exp)
{
    const int h = m / 2, ldv = 2 * S;
    std::fill(Vt.begin(), Vt.end(), T(0));
    for (int i = 0; i < S; i++) Vt[(size_t)i * ldv + 2 * i] = T(1);
    const T thr = std::ldexp(scale, tol_exp);
    std::vector<T> c(h), s(h), wr(h), wi(h);
    std::vector<int> p(h), q(h);
    auto at = [&](int i, int j) { return &Z[2 * ((size_t)i * m + j)]; };
    for (int sweep = 0; sweep < EIG_MAX_SWEEPS; sweep++) {
        bool big = false;
        for (int r = 0; r < m - 1; r++) {
            for (int a = 0; a < h; a++) {
                eig_pair(m, r, a, &p[a], &q[a]);
                const T app = at(p[a], p[a])[0], aqq = at(q[a], q[a])[0];
                T t, mod;
                eig_rotation_c(app, at(p[a], q[a])[0], at(p[a], q[a])[1], aqq, &c[a], &s[a], &t, &wr[a], &wi[a], &mod);
                if (mod != T(0)) {
                    at(p[a], p[a])[0] = eig_fma(-t, mod, app);
                    at(q[a], q[a])[0] = eig_fma(t, mod, aqq);
                    at(p[a], q[a])[0] = at(p[a], q[a])[1] = at(q[a], p[a])[0] = at(q[a], p[a])[1] = T(0);
                    big = big || mod > thr;
                }
            }
            for (int a = 0; a < h; a++) {
                for (int b = 0; b < h; b++) {
                    if (a == b) continue;
                    T *z[4] = {at(p[a], p[b]), at(p[a], q[b]), at(q[a], p[b]), at(q[a], q[b])};
                    T x[8] = {z[0][0], z[0][1], z[1][0], z[1][1], z[2][0], z[2][1], z[3][0], z[3][1]};
                    eig_block_c(a > b, c[a], s[a], wr[a], wi[a], c[b], s[b], wr[b], wi[b], x);
                    for (int e = 0; e < 4; e++) z[e][0] = x[2 * e], z[e][1] = x[2 * e + 1];
                }
                for (int j = 0; j < S; j++) {
                    T *vp = &Vt[(size_t)p[a] * ldv + 2 * j], *vq = &Vt[(size_t)q[a] * ldv + 2 * j];
                    eig_cmul(wr[a], -wi[a], &vq[0], &vq[1]);
                    eig_rot2(c[a], s[a], &vp[0], &vq[0]);
                    eig_rot2(c[a], s[a], &vp[1], &vq[1]);
                }
            }
        }
        if (!big) return true;
    }
    return false;
}

// The law of include/sfe_dsp.h on one problem in float64, rounded once on the way out.  G: n x n float32, only i <= j
// read; a: the band's steering [B][S].  null_spec, vectors may be null.  Returns the status.
int eig_solve_host(int S, int B, int E, int wl, int D, const float *G, const float *a, float *values, float *null_spec, float *vectors)
{
    const int n = 2 * S, m = eig_order(S, wl), nv = wl ? n : S;     // nv eigenvectors kept, a row of Vt each
    const size_t nn = (size_t)n;
    std::vector<double> A(wl ? nn * nn : 2 * (size_t)m * m, 0.0), Vt((size_t)m * nn);
    auto up = [&](size_t i, size_t j) { return (double)(i <= j ? G[i * nn + j] : G[j * nn + i]); };
    bool ok = true;
    double top = 0.0;
    for (size_t s = 0; s < (size_t)S; s++)
        for (size_t t = 0; t < (size_t)S; t++) {
            const double g00 = up(2 * s, 2 * t), g01 = up(2 * s, 2 * t + 1), g10 = up(2 * s + 1, 2 * t), g11 = up(2 * s + 1, 2 * t + 1);
            double e[4];
            if (wl) {
                double *l0 = &A[2 * s * nn + 2 * t], *l1 = l0 + nn;
                e[0] = l0[0] = g00, e[1] = l0[1] = g01, e[2] = l1[0] = g10, e[3] = l1[1] = g11;
            } else {                                        // Z[s][t] = G^[2s][2t] + j G^[2s+1][2t]
                e[0] = e[3] = A[2 * (s * m + t)] = 0.5 * (g00 + g11);
                e[1] = e[2] = A[2 * (s * m + t) + 1] = 0.5 * (g10 - g01);
                ok = ok && std::fabs(g00 + g11) <= (double)FLT_MAX && std::fabs(g10 - g01) <= (double)FLT_MAX;     // float32 forms these first
            }
            for (const double v : e) {
                ok = ok && std::isfinite(v) && std::fabs(v) <= (double)FLT_MAX;     // what float32 holds as finite
                top = std::max(top, std::fabs(v));
            }
        }
    // the threshold's scale: the power of two at or below the largest entry
    if (ok) {
        const double scale = top > 0.0 ? std::ldexp(1.0, std::ilogb(top)) : 1.0;
        ok = wl ? jacobi(A, Vt, n, scale, EIG_TOL_EXP_HOST) : jacobi_c(A, Vt, m, S, scale, EIG_TOL_EXP_HOST);
    }
    const float qnan = std::nanf("");
    if (!ok) {
        for (size_t i = 0; i < nn; i++) values[i] = qnan;
        if (null_spec)
            for (int b = 0; b < B; b++) null_spec[b] = qnan;
        if (vectors)
            for (size_t e = 0; e < 2 * (size_t)E * nn; e++) vectors[e] = (e / nn == e % nn) ? 1.0f : 0.0f;
        return 1;
    }
    const size_t dstep = wl ? nn + 1 : 2 * ((size_t)m + 1);         // from one diagonal entry to the next
    std::vector<int> ord(nv);
    for (int i = 0; i < nv; i++) {
        const double di = A[i * dstep];
        int rank = 0;
        for (int j = 0; j < nv; j++) {
            const double dj = A[j * dstep];
            rank += (dj > di || (dj == di && j < i)) ? 1 : 0;
        }
        ord[rank] = i;
        if (wl) values[rank] = (float)di;
        else values[2 * rank] = values[2 * rank + 1] = (float)di;
        double *v = &Vt[i * nn], ss = 0.0, big = 0.0, at = 1.0;
        for (int j = 0; j < n; j++) {
            ss += v[j] * v[j];
            if (std::fabs(v[j]) > big) big = std::fabs(v[j]), at = v[j];
        }
        const double nrm = at < 0.0 ? -std::sqrt(ss) : std::sqrt(ss);
        for (int j = 0; j < n; j++) v[j] /= nrm;
    }
    if (vectors)
        for (int r = 0; r < 2 * E; r++)
            for (int j = 0; j < n; j++) {
                double v;
                if (wl) {
                    v = Vt[ord[r] * nn + j];
                } else if (!(r & 1)) {
                    v = Vt[ord[r >> 1] * nn + j];
                } else {
                    const double w = Vt[ord[r >> 1] * nn + (j ^ 1)];
                    v = (j & 1) ? w : -w;
                }
                vectors[r * nn + j] = (float)v;
            }
    if (null_spec)
        for (int b = 0; b < B; b++) {
            const float *st = a + (size_t)b * nn;
            double q00 = 0.0, q11 = 0.0, q01 = 0.0, aa = 0.0;
            for (int s = 0; s < S; s++) aa += (double)st[2 * s] * st[2 * s] + (double)st[2 * s + 1] * st[2 * s + 1];
            for (int r = wl ? D : D / 2; r < nv; r++) {
                const double *v = &Vt[ord[r] * nn];
                double x = 0.0, y = 0.0;
                for (int s = 0; s < S; s++) {
                    const double re = st[2 * s], im = st[2 * s + 1];
                    x += v[2 * s] * re + v[2 * s + 1] * im;
                    y += v[2 * s + 1] * re - v[2 * s] * im;
                }
                if (wl) q00 += x * x, q11 += y * y, q01 += x * y;
                else q00 += x * x + y * y, q11 = q00;       // u(w) and u(jw) together: Q = |w^H a|^2 I
            }
            const double mid = 0.5 * (q00 + q11), d = 0.5 * (q00 - q11);
            null_spec[b] = (float)(std::max(mid - std::sqrt(d * d + q01 * q01), 0.0) / aa);
        }
    return 0;
}

}  // namespace
}  // namespace sfe

using namespace sfe;

extern "C" {

int sfe_dsp_eig_plan(int n_in, int n_beams, int n_vec, int n_bands, const float *steering, int widely_linear, int signal_dim,
                     const float *gram, float *values, float *null_spectrum, float *vectors, int *status)
{
    const int rc = eig_check(n_in, n_beams, n_vec, n_bands, steering, widely_linear, signal_dim);
    if (rc != SFE_OK) return rc;
    if (!gram) return SFE_OK;
    if (!values) {
        set_error("eig: null values with a gram to decompose");
        return SFE_EINVAL;
    }
    const size_t n = 2 * (size_t)n_in, B = (size_t)n_beams, E = (size_t)n_vec;
    for (size_t k = 0; k < (size_t)n_bands; k++) {
        const int st = eig_solve_host(n_in, n_beams, n_vec, widely_linear, signal_dim, gram + k * n * n, B ? steering + k * B * n : nullptr,
                                      values + k * n, null_spectrum ? null_spectrum + k * B : nullptr,
                                      vectors ? vectors + k * 2 * E * n : nullptr);
        if (status) status[k] = st;
    }
    return SFE_OK;
}

int sfe_dsp_eig_create(const float *steering, int n_in, int n_beams, int n_vec, int n_bands, int widely_linear, int signal_dim,
                       int device, sfe_eig_t *out)
{
    if (!out) return SFE_EINVAL;
    *out = nullptr;
    int rc = eig_check(n_in, n_beams, n_vec, n_bands, steering, widely_linear, signal_dim);
    if (rc != SFE_OK) return rc;
    CreateScope scope(device);
    if (scope.rc != SFE_OK) return scope.rc;
    std::unique_ptr<Eig> p(new (std::nothrow) Eig);
    if (!p) return SFE_ENOMEM;
    p->S = n_in;
    p->B = n_beams;
    p->E = n_vec;
    p->M = n_bands;
    p->wl = widely_linear;
    p->D = signal_dim;
    p->device = device;
    if (n_beams && (rc = p->d_steer.upload(steering, (size_t)n_bands * n_beams * n_in * 2)) != SFE_OK) return rc;
    SFE_HIP(hipDeviceSynchronize());
    *out = p.release();
    return SFE_OK;
}

int sfe_dsp_eig_set_steering(sfe_eig_t h, const float *steering)
{
    Eig *p = as_eig(h);
    if (!p) return SFE_EINVAL;
    if (p->B == 0) {
        set_error("eig: set_steering on a handle of no beams");
        return SFE_EINVAL;
    }
    const int rc = eig_check_steering(p->S, p->B, p->M, steering);
    if (rc != SFE_OK) return rc;
    SFE_ON_DEVICE(p->device);
    // calls already enqueued read the table: they finish with the old one before it is replaced
    SFE_HIP(hipDeviceSynchronize());
    SFE_HIP(hipMemcpy(p->d_steer, steering, (size_t)p->M * p->B * p->S * 2 * sizeof(float), hipMemcpyHostToDevice));
    SFE_HIP(hipDeviceSynchronize());
    return SFE_OK;
}

int sfe_dsp_eig_set_signal_dim(sfe_eig_t h, int signal_dim)
{
    Eig *p = as_eig(h);
    if (!p) return SFE_EINVAL;
    const int rc = eig_check_signal_dim(p->S, p->wl, signal_dim);
    if (rc != SFE_OK) return rc;
    p->D = signal_dim;          // a call takes it by value when it is enqueued
    return SFE_OK;
}

int sfe_dsp_eig_process_stream(sfe_eig_t h, const void *d_gram, size_t n_rows, size_t in_stride, void *d_values, size_t values_stride,
                               void *d_null, size_t null_stride, void *d_vectors, size_t vectors_stride, void *d_status,
                               size_t status_stride, size_t *n_out, sfe_stream_t stream)
{
    static const char who[] = "eig_process_stream";
    Eig *p = stream_handle(as_eig(h), who, n_out);
    if (!p) return SFE_EINVAL;
    const size_t M = (size_t)p->M, B = (size_t)p->B, n2 = 2 * (size_t)p->S, gram = n2 * n2, mat = 2 * (size_t)p->E * n2;
    if (n_rows >= ((size_t)1 << 31) / gram) {
        set_error("eig_process_stream: n_rows = %zu must be below 2^31 / (2 n_in)^2 = %zu per call", n_rows, ((size_t)1 << 31) / gram);
        return SFE_EINVAL;
    }
    if (n_rows == 0) return SFE_OK;
    int rc = refuse_null(who, {d_gram, d_values});
    if (rc != SFE_OK) return rc;
    if (B == 0) d_null = nullptr;           // nothing to write
    if (mat == 0) d_vectors = nullptr;
    if (values_stride < M * n2 || (d_null && null_stride < M * B) || (d_vectors && vectors_stride < M * mat) ||
        (d_status && status_stride < M)) {
        set_error("eig_process_stream: values_stride %zu < n_bands * 2 n_in = %zu, null_stride %zu < n_bands * n_beams = %zu, "
                  "vectors_stride %zu < n_bands * 4 n_vec n_in = %zu or status_stride %zu < n_bands = %zu",
                  values_stride, M * n2, null_stride, M * B, vectors_stride, M * mat, status_stride, M);
        return SFE_ERANGE;
    }
    if (in_stride < n_rows * gram) {
        set_error("eig_process_stream: in_stride %zu < n_rows * (2 n_in)^2 = %zu", in_stride, n_rows * gram);
        return SFE_EINVAL;
    }
    Span in, o[4];      // the values, the null spectrum, the vectors, the status
    if (!solver_ranges(M, d_gram, n_rows, in_stride, gram,
                       {RowOut{d_values, values_stride, M * n2}, RowOut{d_null, null_stride, M * B}, RowOut{d_vectors, vectors_stride, M * mat},
                        RowOut{d_status, status_stride, M}},
                       &in, o))
        return refuse_2_62(who);
    hipStream_t s = (hipStream_t)stream;
    if ((rc = refuse_misaligned(who, "float32 and int32 4 B", {in, o[0], o[1], o[2], o[3]})) != SFE_OK ||
        (rc = refuse_overlap(who, in, {o[0], o[1], o[2], o[3]})) != SFE_OK)
        return rc;
    if (stream_is_capturing(s)) {       // set_steering may replace the table a captured call would have pinned
        set_error("eig_process_stream: graph capture is not supported (set_steering may replace the steering table)");
        return SFE_ESTATE;
    }
    SFE_ON_DEVICE(p->device);
    const EigArgs a{static_cast<const float *>(d_gram), p->d_steer, static_cast<float *>(d_values), static_cast<float *>(d_null),
                    static_cast<float *>(d_vectors), static_cast<int *>(d_status), (long long)in_stride, (long long)values_stride,
                    (long long)null_stride, (long long)vectors_stride, (long long)status_stride, p->S, p->B, p->E, p->M, p->D};
    rc = launch_eig(a, p->wl, (long long)n_rows, s);
    if (rc != SFE_OK) return rc;
    *n_out = n_rows;
    return SFE_OK;
}

int sfe_dsp_eig_destroy(sfe_eig_t h) { return destroy_handle(as_eig(h)); }

}  // extern "C"
