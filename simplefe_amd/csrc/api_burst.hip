// api_burst.hip -- the burst-demodulator handle behind sfe_burst_t, sfe_dsp_burst_* (include/sfe_dsp.h).  Host code only;
// the kernel is in burst.hip.  Here: the checks and the float64 twin of the kernel's law (sfe_dsp_burst_plan: the CPU
// fallback and what the host tests pin against numpy).
#include <cfloat>
#include <cmath>

#include "host.h"
#include "block.h"
#include "burst.h"

namespace sfe {
namespace {

struct Burst {
    static constexpr uint32_t MAGIC = 0x42525331u;   // 'BRS1'
    uint32_t magic = MAGIC;
    int sps = 0, N = 0, Lp = 0, lag = 0, fixed_timing = 0, n_streams = 1, device = 0, in_u8 = 0;
    float E_p = 0.0f, min_gate = 0.0f;
    DevBuf<v2f> d_pre;              // [Lp]
    DevBuf<v2f> d_tw;               // [sps]: exp(-j 2 pi r / sps)
};

Burst *as_burst(void *h) { return as_handle<Burst>(h, "burst-demodulator"); }

int burst_check_gate(float min_gate)
{
    if (!std::isfinite(min_gate)) {
        set_error("burst: min_gate must be finite");
        return SFE_EINVAL;
    }
    return SFE_OK;
}

// *E_p: sum |p|^2 formed in float64 and rounded once
int burst_check(const float *pre, int Lp, int sps, int N, int lag, int timing_mode, float min_gate, int n_streams, float *E_p)
{
    if (sps < BURST_MIN_SPS || sps > BURST_MAX_SPS) {
        set_error("burst: sps = %d must be in [%d, %d]", sps, BURST_MIN_SPS, BURST_MAX_SPS);
        return SFE_EINVAL;
    }
    if (N < BURST_MIN_SYM || N > BURST_MAX_SYM) {
        set_error("burst: n_sym = %d must be in [%d, %d]", N, BURST_MIN_SYM, BURST_MAX_SYM);
        return SFE_EINVAL;
    }
    if (Lp < 2 || Lp > N) {
        set_error("burst: n_pre = %d must be in [2, n_sym = %d]", Lp, N);
        return SFE_EINVAL;
    }
    if (lag < 1 || lag >= Lp) {
        set_error("burst: lag = %d must be in [1, n_pre - 1 = %d]", lag, Lp - 1);
        return SFE_EINVAL;
    }
    if (timing_mode != 0 && timing_mode != 1) {
        set_error("burst: timing_mode = %d must be 0 (estimate) or 1 (tau = 0)", timing_mode);
        return SFE_EINVAL;
    }
    if (n_streams < 1) {
        set_error("burst: n_streams = %d must be at least 1", n_streams);
        return SFE_EINVAL;
    }
    const int rc = burst_check_gate(min_gate);
    if (rc != SFE_OK) return rc;
    if (!pre) {
        set_error("burst: null preamble");
        return SFE_EINVAL;
    }
    double e = 0.0;
    for (int k = 0; k < 2 * Lp; k++) {
        if (!std::isfinite(pre[k])) {
            set_error("burst: preamble value %d is not finite", k / 2);
            return SFE_EINVAL;
        }
        e += (double)pre[k] * pre[k];
    }
    if (!((float)e > 0.0f) || !std::isfinite((float)e)) {
        set_error("burst: the preamble's energy must be positive and finite in float32");
        return SFE_EINVAL;
    }
    *E_p = (float)e;
    return SFE_OK;
}

bool usable(double re, double im) { return std::isfinite(re) && std::isfinite(im) && (re != 0.0 || im != 0.0); }

void unturn(double t, double *c, double *s)     // exp(-j 2 pi t) as (c, s)
{
    t -= std::rint(t);
    *c = std::cos(2.0 * M_PI * t);
    *s = -std::sin(2.0 * M_PI * t);
}

// The law of include/sfe_dsp.h on one burst in float64, rounded once on the way out.  x: the reach, (N + 2) sps cf32
// samples from o - sps on.  The estimates are rounded to float32 where the law hands them on, as the record holds them.
// given: tau, f, theta, a to take instead of estimating, or null.  Returns the status.
int burst_solve_host(int sps, int N, int Lp, int lag, int fixed_timing, float E_p, const float *pre, const float *x, const float *given,
                     float *sym, float *rec)
{
    const size_t reach = ((size_t)N + 2) * sps;
    auto fail = [&]() {
        for (int k = 0; k < 2 * N; k++) sym[k] = 0.0f;
        if (rec)
            for (int i = 0; i < BURST_REC; i++) rec[i] = i < 6 ? std::nanf("") : 0.0f;
        return BURST_NO_ESTIMATE;
    };
    for (size_t i = 0; i < 2 * reach; i++)
        if (!std::isfinite(x[i])) return fail();
    float tau = 0.0f, f = 0.0f, theta = 0.0f, amp = 0.0f;
    if (given) {
        tau = given[0], f = given[1], theta = given[2], amp = given[3];
        if (!(std::isfinite(tau) && std::fabs(tau) <= 0.5f * sps && std::isfinite(f) && std::isfinite(theta) && amp > 0.0f && std::isfinite(amp)))
            return fail();
    } else if (!fixed_timing) {
        double cr = 0.0, ci = 0.0;
        for (size_t i = 0; i < (size_t)N * sps; i++) {
            const double re = x[2 * (sps + i)], im = x[2 * (sps + i) + 1], p = re * re + im * im, ang = 2.0 * M_PI * (double)(i % sps) / sps;
            cr += p * std::cos(ang);
            ci -= p * std::sin(ang);
        }
        if (!usable(cr, ci)) return fail();
        double t = 0.0 - sps * (std::atan2(ci, cr) / (2.0 * M_PI));
        if (t <= -0.5 * sps) t += sps;
        tau = (float)t;
    }
    const int m = (int)std::floor((double)tau);
    const double mu = (double)tau - m;
    const double L[4] = {-mu * (mu - 1.0) * (mu - 2.0) / 6.0, (mu + 1.0) * (mu - 1.0) * (mu - 2.0) / 2.0, -(mu + 1.0) * mu * (mu - 2.0) / 2.0,
                         (mu + 1.0) * mu * (mu - 1.0) / 6.0};
    std::vector<double> y(2 * (size_t)N), z(2 * (size_t)Lp);
    double ey = 0.0;
    for (int k = 0; k < N; k++) {
        const float *v = x + 2 * ((size_t)sps + (size_t)k * sps + m - 1);
        double yr = 0.0, yi = 0.0;
        for (int q = 0; q < 4; q++) yr += L[q] * v[2 * q], yi += L[q] * v[2 * q + 1];
        y[2 * k] = yr, y[2 * k + 1] = yi;
        if (k < Lp) {
            const double pr = pre[2 * k], pi = pre[2 * k + 1];
            z[2 * k] = yr * pr + yi * pi, z[2 * k + 1] = yi * pr - yr * pi;
            ey += yr * yr + yi * yi;
        }
    }
    double S2 = 0.0;
    if (!given || rec) {
        double Rr = 0.0, Ri = 0.0;
        for (int k = 0; k + lag < Lp; k++) {
            const double ur = z[2 * (k + lag)], ui = z[2 * (k + lag) + 1], vr = z[2 * k], vi = z[2 * k + 1];
            Rr += ur * vr + ui * vi, Ri += ui * vr - ur * vi;
        }
        if (!given) {
            if (!usable(Rr, Ri)) return fail();
            f = (float)(std::atan2(Ri, Rr) / (2.0 * M_PI * lag));
        }
        double Sr = 0.0, Si = 0.0;
        for (int k = 0; k < Lp; k++) {
            double c, s;
            unturn((double)f * k, &c, &s);
            Sr += z[2 * k] * c - z[2 * k + 1] * s, Si += z[2 * k + 1] * c + z[2 * k] * s;
        }
        S2 = Sr * Sr + Si * Si;
        if (!given) {
            if (!usable(Sr, Si)) return fail();
            theta = (float)(std::atan2(Si, Sr) / (2.0 * M_PI));
            amp = (float)(std::sqrt(S2) / (double)E_p);
            if (!(amp > 0.0f) || !std::isfinite(amp)) return fail();
        }
    }
    double ev = 0.0;
    for (int k = 0; k < N; k++) {
        double c, s;
        unturn((double)theta + (double)f * k, &c, &s);
        const double wr = (y[2 * k] * c - y[2 * k + 1] * s) / (double)amp, wi = (y[2 * k + 1] * c + y[2 * k] * s) / (double)amp;
        sym[2 * k] = (float)wr, sym[2 * k + 1] = (float)wi;
        if (k < Lp) {
            const double dr = wr - pre[2 * k], di = wi - pre[2 * k + 1];
            ev += dr * dr + di * di;
        }
    }
    if (rec) {
        rec[0] = tau, rec[1] = f, rec[2] = theta, rec[3] = amp;
        rec[4] = (float)(S2 / ((double)E_p * ey));
        rec[5] = (float)(ev / (double)E_p);
        rec[6] = rec[7] = 0.0f;
    }
    return BURST_OK;
}

}  // namespace
}  // namespace sfe

using namespace sfe;

extern "C" {

int sfe_dsp_burst_plan(const float *preamble, int n_pre, int sps, int n_sym, int lag, int timing_mode, float min_gate, const float *x,
                       size_t n_in, const uint32_t *idx, const float *gate, size_t n_bursts, int64_t start_base, int64_t start_step,
                       const float *given, float *symbols, float *record, int *status)
{
    float E_p = 0.0f;
    const int rc = burst_check(preamble, n_pre, sps, n_sym, lag, timing_mode, min_gate, 1, &E_p);
    if (rc != SFE_OK) return rc;
    if (!x || n_bursts == 0) return SFE_OK;
    if (!symbols) {
        set_error("burst: null symbols with samples to demodulate");
        return SFE_EINVAL;
    }
    if (n_in >= ((size_t)1 << 31)) {
        set_error("burst: n_in = %zu must be below 2^31", n_in);
        return SFE_EINVAL;
    }
    if (n_bursts >= ((size_t)1 << 31)) {
        set_error("burst: n_bursts = %zu must be below 2^31", n_bursts);
        return SFE_EINVAL;
    }
    const int rs = check_starts("burst", start_base, start_step, n_bursts);
    if (rs != SFE_OK) return rs;
    const long long reach = ((long long)n_sym + 2) * sps;
    for (size_t b = 0; b < n_bursts; b++) {
        float *sym = symbols + b * 2 * (size_t)n_sym, *rec = record ? record + b * BURST_REC : nullptr;
        int st = BURST_OK;
        const long long o = (long long)start_base + (long long)b * (long long)start_step + (idx ? (long long)idx[b] : 0LL);
        if (gate && !(gate[b] >= min_gate)) st = BURST_GATED;
        else if (o < sps || o - sps > (long long)n_in - reach) st = BURST_OUT_OF_RANGE;
        if (st != BURST_OK) {
            for (int k = 0; k < 2 * n_sym; k++) sym[k] = 0.0f;
            if (rec)
                for (int i = 0; i < BURST_REC; i++) rec[i] = i < 6 ? std::nanf("") : 0.0f;
        } else {
            st = burst_solve_host(sps, n_sym, n_pre, lag, timing_mode, E_p, preamble, x + 2 * (size_t)(o - sps),
                                  given ? given + b * BURST_REC : nullptr, sym, rec);
        }
        if (status) status[b] = st;
    }
    return SFE_OK;
}

int sfe_dsp_burst_create(const float *preamble, int n_pre, int sps, int n_sym, int lag, int timing_mode, float min_gate, int n_streams,
                         int device, sfe_burst_t *out)
{
    if (!out) return SFE_EINVAL;
    *out = nullptr;
    float E_p = 0.0f;
    int rc = burst_check(preamble, n_pre, sps, n_sym, lag, timing_mode, min_gate, n_streams, &E_p);
    if (rc != SFE_OK) return rc;
    CreateScope scope(device);
    if (scope.rc != SFE_OK) return scope.rc;
    std::unique_ptr<Burst> p(new (std::nothrow) Burst);
    if (!p) return SFE_ENOMEM;
    p->sps = sps;
    p->N = n_sym;
    p->Lp = n_pre;
    p->lag = lag;
    p->fixed_timing = timing_mode;
    p->n_streams = n_streams;
    p->device = device;
    p->E_p = E_p;
    p->min_gate = min_gate;
    std::vector<v2f> tw(sps);
    for (int r = 0; r < sps; r++) {
        const double ang = 2.0 * M_PI * r / sps;
        tw[r] = v2f{(float)cos(ang), (float)-sin(ang)};
    }
    tw[0] = v2f{1.0f, 0.0f};        // +0, not -0
    if ((rc = p->d_pre.upload(reinterpret_cast<const v2f *>(preamble), (size_t)n_pre)) != SFE_OK || (rc = p->d_tw.upload(tw)) != SFE_OK) return rc;
    SFE_HIP(hipDeviceSynchronize());
    *out = p.release();
    return SFE_OK;
}

int sfe_dsp_burst_set_input_format(sfe_burst_t h, int fmt)
{
    return set_format(as_burst(h), "burst_set_input_format", fmt, SFE_FMT_U8, "SFE_FMT_U8", &Burst::in_u8);
}

int sfe_dsp_burst_set_gate(sfe_burst_t h, float min_gate)
{
    Burst *p = as_burst(h);
    if (!p) return SFE_EINVAL;
    const int rc = burst_check_gate(min_gate);
    if (rc != SFE_OK) return rc;
    p->min_gate = min_gate;         // a call takes it by value when it is enqueued
    return SFE_OK;
}

int sfe_dsp_burst_process_stream(sfe_burst_t h, const void *d_in, size_t n_in, size_t in_stride, const void *d_idx, size_t idx_stride,
                                 const void *d_gate, size_t gate_stride, size_t n_bursts, int64_t start_base, int64_t start_step, void *d_out,
                                 size_t out_stride, void *d_rec, void *d_status, size_t status_stride, size_t *n_out, sfe_stream_t stream)
{
    static const char who[] = "burst_process_stream";
    Burst *p = stream_handle(as_burst(h), who, n_out);
    if (!p) return SFE_EINVAL;
    bool go;
    int rc = check_windows(who, "n_sym", (size_t)p->n_streams, p->in_u8 ? 2 : 8, d_in, n_in, in_stride, d_idx, idx_stride, d_gate, gate_stride,
                           n_bursts, start_base, start_step, d_out, out_stride, (size_t)p->N, nullptr, 0, d_rec, BURST_REC, d_status,
                           status_stride, &go);
    if (rc != SFE_OK || !go) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (stream_is_capturing(s)) {       // set_gate may change what a captured call would have pinned
        set_error("burst_process_stream: graph capture is not supported (set_gate may change the gate a captured call would have pinned)");
        return SFE_ESTATE;
    }
    SFE_ON_DEVICE(p->device);
    const BurstArgs a{d_in, static_cast<const unsigned *>(d_idx), static_cast<const float *>(d_gate), p->d_pre, p->d_tw,
                      static_cast<v2f *>(d_out), static_cast<float *>(d_rec), static_cast<int *>(d_status), (long long)in_stride,
                      (long long)idx_stride, (long long)gate_stride, (long long)out_stride, (long long)status_stride, (long long)n_in,
                      (long long)n_bursts, (long long)start_base, (long long)start_step, p->E_p, p->min_gate, p->sps, p->N, p->Lp, p->lag,
                      p->fixed_timing, burst_staged(p->sps, p->N, p->Lp) ? 1 : 0};
    rc = launch_burst(a, p->in_u8, p->n_streams, s);
    if (rc != SFE_OK) return rc;
    *n_out = n_bursts;
    return SFE_OK;
}

int sfe_dsp_burst_destroy(sfe_burst_t h) { return destroy_handle(as_burst(h)); }

}  // extern "C"
