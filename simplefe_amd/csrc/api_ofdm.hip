// api_ofdm.hip -- the OFDM-receiver handle behind sfe_ofdm_t, sfe_dsp_ofdm_* (include/sfe_dsp.h).  Host code only; the
// kernel is in ofdm.hip.  Here: the checks, the tables of a shape and the float64 twin of the kernel's law
// (sfe_dsp_ofdm_plan: the CPU fallback and what the host tests pin against numpy).
#include <cfloat>
#include <cmath>

#include "host.h"
#include "block.h"
#include "ofdm.h"

namespace sfe {
namespace {

// a checked shape and the tables both the plan and the handle read
struct OfdmShape {
    int logn = 0, N = 0, cp = 0, g = 0, T = 0, Ns = 0, Nd = 0, Np = 0, cfo = 0, q = 0, mrc = 0;
    float min_gate = 0.0f, pilot_den = 0.0f;
    std::vector<v2f> c, pilot;          // [N]: conj(train) / (T |train|^2) on used bins, +0 elsewhere; the pilots, +0 off their bins
    std::vector<float> sign;            // [Ns]
    std::vector<int> bins;              // the Nd data bins, then the Np pilot bins, each in increasing k
};

struct Ofdm {
    static constexpr uint32_t MAGIC = 0x4f46444du;   // 'OFDM'
    uint32_t magic = MAGIC;
    int n_streams = 1, device = 0, in_u8 = 0;
    OfdmShape sh;
    DevBuf<v2f> d_tw, d_c, d_pilot;     // [N] each
    DevBuf<float> d_sign;               // [Ns]
    DevBuf<int> d_bins;                 // [Nu]
};

Ofdm *as_ofdm(void *h) { return as_handle<Ofdm>(h, "OFDM-receiver"); }

#define OFDM_REFUSE(...)            \
    do {                            \
        set_error(__VA_ARGS__);     \
        return SFE_EINVAL;          \
    } while (0)

int ofdm_check(int n_fft, int cp, int advance, int n_train, int n_data, const uint8_t *kind, const float *train, const float *pilot,
               const int8_t *pilot_sign, int cfo_mode, int cfo_skip, int out_mode, float min_gate, int n_streams, OfdmShape *sh)
{
    int logn = 0;
    while (logn < 31 && (1 << logn) < n_fft) logn++;
    if (n_fft < (1 << OFDM_MIN_LOGN) || n_fft > (1 << OFDM_MAX_LOGN) || (1 << logn) != n_fft)
        OFDM_REFUSE("ofdm: n_fft = %d must be a power of two in [%d, %d]", n_fft, 1 << OFDM_MIN_LOGN, 1 << OFDM_MAX_LOGN);
    if (cp < 0 || cp > n_fft) OFDM_REFUSE("ofdm: cp = %d must be in [0, n_fft = %d]", cp, n_fft);
    if (advance < 0 || advance > cp) OFDM_REFUSE("ofdm: advance = %d must be in [0, cp = %d]", advance, cp);
    if (n_train < 1 || n_train > OFDM_MAX_TRAIN) OFDM_REFUSE("ofdm: n_train = %d must be in [1, %d]", n_train, OFDM_MAX_TRAIN);
    if (n_data < 1 || n_data > OFDM_MAX_DATA) OFDM_REFUSE("ofdm: n_data = %d must be in [1, %d]", n_data, OFDM_MAX_DATA);
    if ((long long)(n_train + n_data) * (n_fft + cp) >= (1LL << 31))
        OFDM_REFUSE("ofdm: (n_train + n_data) * (n_fft + cp) = %lld must be below 2^31", (long long)(n_train + n_data) * (n_fft + cp));
    if (cfo_mode != 0 && cfo_mode != 1) OFDM_REFUSE("ofdm: cfo_mode = %d must be 0 (none) or 1 (from the cyclic prefix)", cfo_mode);
    if (cfo_mode == 1 && cp < 1) OFDM_REFUSE("ofdm: cfo_mode 1 needs cp >= 1");
    if (cfo_mode == 0 ? cfo_skip != 0 : (cfo_skip < 0 || cfo_skip >= cp))
        OFDM_REFUSE("ofdm: cfo_skip = %d must be in [0, cp = %d), and 0 with cfo_mode 0", cfo_skip, cp);
    if (out_mode != SFE_OFDM_OUT_ZF && out_mode != SFE_OFDM_OUT_MRC)
        OFDM_REFUSE("ofdm: out_mode = %d must be SFE_OFDM_OUT_ZF (0) or SFE_OFDM_OUT_MRC (1)", out_mode);
    if (!std::isfinite(min_gate)) OFDM_REFUSE("ofdm: min_gate must be finite");
    if (n_streams < 1) OFDM_REFUSE("ofdm: n_streams = %d must be at least 1", n_streams);
    if (!kind || !train) OFDM_REFUSE("ofdm: null kind or train table");
    const int N = n_fft;
    std::vector<int> data, pil;
    for (int k = 0; k < N; k++) {
        if (kind[k] > OFDM_PILOT) OFDM_REFUSE("ofdm: kind[%d] = %d must be 0 (null), 1 (data) or 2 (pilot)", k, (int)kind[k]);
        if (kind[k] == OFDM_DATA) data.push_back(k);
        if (kind[k] == OFDM_PILOT) pil.push_back(k);
    }
    if (data.empty()) OFDM_REFUSE("ofdm: kind names no data bin");
    if (!pil.empty() && !pilot) OFDM_REFUSE("ofdm: null pilot table with %zu pilot bins", pil.size());
    sh->c.assign(N, v2f{0.0f, 0.0f});
    sh->pilot.assign(N, v2f{0.0f, 0.0f});
    double pe = 0.0;
    for (int k = 0; k < N; k++) {
        const float tr = train[2 * k], ti = train[2 * k + 1];
        if (!std::isfinite(tr) || !std::isfinite(ti)) OFDM_REFUSE("ofdm: train value %d is not finite", k);
        if (pilot && (!std::isfinite(pilot[2 * k]) || !std::isfinite(pilot[2 * k + 1]))) OFDM_REFUSE("ofdm: pilot value %d is not finite", k);
        if (kind[k] == OFDM_NULL) continue;
        const double e = (double)tr * tr + (double)ti * ti;
        const v2f c = v2f{(float)((double)tr / (n_train * e)), (float)(-(double)ti / (n_train * e))};
        if (!(e > 0.0) || !std::isfinite(c.x) || !std::isfinite(c.y) || (c.x == 0.0f && c.y == 0.0f))
            OFDM_REFUSE("ofdm: train value %d of a used bin is zero, or its inverse leaves float32", k);
        sh->c[k] = c;
        if (kind[k] == OFDM_PILOT) {
            const double p = (double)pilot[2 * k] * pilot[2 * k] + (double)pilot[2 * k + 1] * pilot[2 * k + 1];
            if (!(p > 0.0)) OFDM_REFUSE("ofdm: pilot value %d of a pilot bin is zero", k);
            sh->pilot[k] = v2f{pilot[2 * k], pilot[2 * k + 1]};
            pe += p;
        }
    }
    sh->sign.assign(n_data, 1.0f);
    for (int j = 0; pilot_sign && j < n_data; j++) {
        if (pilot_sign[j] != 1 && pilot_sign[j] != -1) OFDM_REFUSE("ofdm: pilot_sign[%d] = %d must be +1 or -1", j, (int)pilot_sign[j]);
        sh->sign[j] = (float)pilot_sign[j];
    }
    sh->pilot_den = (float)(pe * n_data);
    if (!pil.empty() && !std::isfinite(sh->pilot_den)) OFDM_REFUSE("ofdm: the pilots' energy leaves float32");
    sh->logn = logn, sh->N = N, sh->cp = cp, sh->g = advance, sh->T = n_train, sh->Ns = n_data;
    sh->Nd = (int)data.size(), sh->Np = (int)pil.size();
    sh->cfo = cfo_mode, sh->q = cfo_skip, sh->mrc = out_mode == SFE_OFDM_OUT_MRC, sh->min_gate = min_gate;
    sh->bins = data;
    sh->bins.insert(sh->bins.end(), pil.begin(), pil.end());
    return SFE_OK;
}

bool usable(double re, double im) { return std::isfinite(re) && std::isfinite(im) && (re != 0.0 || im != 0.0); }

// in-place radix-2 transform of N = 2^logn points, exp(-j 2 pi k n / N), every twiddle from cos and sin in float64
void dft64(int logn, std::vector<double> &re, std::vector<double> &im, const std::vector<double> &wr, const std::vector<double> &wi)
{
    const int N = 1 << logn;
    for (int i = 0, j = 0; i < N; i++) {
        if (i < j) std::swap(re[i], re[j]), std::swap(im[i], im[j]);
        int m = N >> 1;
        for (; m >= 1 && (j & m); m >>= 1) j ^= m;
        j |= m;
    }
    for (int len = 2; len <= N; len <<= 1) {
        const int half = len >> 1, step = N / len;
        for (int i = 0; i < N; i += len)
            for (int k = 0; k < half; k++) {
                const double cr = wr[k * step], ci = wi[k * step], ur = re[i + k], ui = im[i + k];
                const double tr = re[i + k + half] * cr - im[i + k + half] * ci, ti = im[i + k + half] * cr + re[i + k + half] * ci;
                re[i + k] = ur + tr, im[i + k] = ui + ti;
                re[i + k + half] = ur - tr, im[i + k + half] = ui - ti;
            }
    }
}

void ofdm_fail_host(const OfdmShape &sh, float *sym, float *chan, float *rec)
{
    for (size_t k = 0; k < 2 * (size_t)sh.Ns * sh.Nd; k++) sym[k] = 0.0f;
    if (chan)
        for (int k = 0; k < 2 * sh.N; k++) chan[k] = 0.0f;
    if (rec)
        for (int i = 0; i < OFDM_REC; i++) rec[i] = i < 6 ? std::nanf("") : 0.0f;
}

// The law of include/sfe_dsp.h on one burst in float64, rounded once on the way out.  x: the reach, (T + Ns)(N + cp) cf32
// samples from o on.  eps, H and phi_j are rounded to float32 where the law hands them on.  Returns the status.
int ofdm_solve_host(const OfdmShape &sh, const std::vector<double> &wr, const std::vector<double> &wi, const float *x, float *sym,
                    float *chan, float *rec)
{
    const int N = sh.N, L = N + sh.cp, nsym = sh.T + sh.Ns, Nd = sh.Nd, Np = sh.Np, Nu = Nd + Np;
    auto fail = [&]() {
        ofdm_fail_host(sh, sym, chan, rec);
        return OFDM_NO_ESTIMATE;
    };
    for (size_t i = 0; i < 2 * (size_t)nsym * L; i++)
        if (!std::isfinite(x[i])) return fail();
    float eps = 0.0f;
    if (sh.cfo) {
        double gr = 0.0, gi = 0.0;
        for (int j = 0; j < nsym; j++)
            for (int i = sh.q; i < sh.cp; i++) {
                const float *v = x + 2 * ((size_t)j * L + i), *u = v + 2 * (size_t)N;
                gr += (double)u[0] * v[0] + (double)u[1] * v[1];
                gi += (double)u[1] * v[0] - (double)u[0] * v[1];
            }
        if (!usable(gr, gi)) return fail();
        eps = (float)(std::atan2(gi, gr) / (2.0 * M_PI));
    }
    std::vector<double> yr(N), yi(N), hr(N, 0.0), hi(N, 0.0);
    auto transform = [&](int j) {
        const size_t n0 = (size_t)j * L + sh.cp - sh.g;
        for (int m = 0; m < N; m++) {
            const double re = x[2 * (n0 + m)], im = x[2 * (n0 + m) + 1];
            if (sh.cfo) {
                double t = (double)eps * (double)(n0 + m) / (double)N;
                t -= std::rint(t);
                const double c = std::cos(2.0 * M_PI * t), s = -std::sin(2.0 * M_PI * t);
                yr[m] = re * c - im * s, yi[m] = im * c + re * s;
            } else {
                yr[m] = re, yi[m] = im;
            }
        }
        dft64(sh.logn, yr, yi, wr, wi);
    };
    for (int j = 0; j < sh.T; j++) {
        transform(j);
        for (int k : sh.bins) {
            const double cr = sh.c[k].x, ci = sh.c[k].y;
            hr[k] += yr[k] * cr - yi[k] * ci, hi[k] += yi[k] * cr + yr[k] * ci;
        }
    }
    double hsum = 0.0, hmin = HUGE_VAL;
    for (int k : sh.bins) {
        hr[k] = (double)(float)hr[k], hi[k] = (double)(float)hi[k];
        const double p = hr[k] * hr[k] + hi[k] * hi[k];
        if (!((float)p > 0.0f) || !std::isfinite((float)p)) return fail();
        hsum += p;
        hmin = std::min(hmin, p);
    }
    const double h2 = hsum / Nu;
    double perr = 0.0, a0 = 0.0, a1 = 0.0;
    for (int j = 0; j < sh.Ns; j++) {
        transform(sh.T + j);
        double pr = 1.0, pi = 0.0;
        const double sg = sh.sign[j];
        if (Np > 0) {
            double Pr = 0.0, Pi = 0.0;
            for (int i = 0; i < Np; i++) {
                const int k = sh.bins[Nd + i];
                const double qr = (hr[k] * sh.pilot[k].x - hi[k] * sh.pilot[k].y) * sg, qi = (hi[k] * sh.pilot[k].x + hr[k] * sh.pilot[k].y) * sg;
                Pr += yr[k] * qr + yi[k] * qi, Pi += yi[k] * qr - yr[k] * qi;
            }
            if (!usable(Pr, Pi)) return fail();
            const double mag = std::hypot(Pr, Pi);
            pr = (double)(float)(Pr / mag), pi = (double)(float)(Pi / mag);
            if (!std::isfinite(pr) || !std::isfinite(pi)) return fail();
        }
        if (j == 0) a0 = std::atan2(pi, pr) / (2.0 * M_PI);
        if (j == sh.Ns - 1) a1 = std::atan2(pi, pr) / (2.0 * M_PI);
        for (int i = 0; i < Nu; i++) {
            const int k = sh.bins[i];
            const double wr_ = hr[k] * pr - hi[k] * pi, wi_ = hi[k] * pr + hr[k] * pi, p = hr[k] * hr[k] + hi[k] * hi[k];
            const double zr = yr[k] * wr_ + yi[k] * wi_, zi = yi[k] * wr_ - yr[k] * wi_;
            if (i < Nd) {
                const double den = sh.mrc ? h2 : p;
                sym[2 * ((size_t)j * Nd + i)] = (float)(zr / den), sym[2 * ((size_t)j * Nd + i) + 1] = (float)(zi / den);
            } else {
                const double dr = zr / p - sh.pilot[k].x * sg, di = zi / p - sh.pilot[k].y * sg;
                perr += dr * dr + di * di;
            }
        }
    }
    if (chan)
        for (int k = 0; k < N; k++) chan[2 * k] = (float)hr[k], chan[2 * k + 1] = (float)hi[k];
    if (rec) {
        rec[0] = eps, rec[1] = (float)h2, rec[2] = (float)(hmin / h2);
        rec[3] = Np > 0 ? (float)(perr / (double)sh.pilot_den) : 0.0f;
        rec[4] = (float)a0, rec[5] = (float)a1;
        rec[6] = rec[7] = 0.0f;
    }
    return OFDM_OK;
}

}  // namespace
}  // namespace sfe

using namespace sfe;

extern "C" {

int sfe_dsp_ofdm_plan(int n_fft, int cp, int advance, int n_train, int n_data, const uint8_t *kind, const float *train, const float *pilot,
                      const int8_t *pilot_sign, int cfo_mode, int cfo_skip, int out_mode, float min_gate, const float *x, size_t n_in,
                      const uint32_t *idx, const float *gate, size_t n_bursts, int64_t start_base, int64_t start_step, float *symbols,
                      float *chan, float *record, int *status)
{
    OfdmShape sh;
    const int rc = ofdm_check(n_fft, cp, advance, n_train, n_data, kind, train, pilot, pilot_sign, cfo_mode, cfo_skip, out_mode, min_gate, 1, &sh);
    if (rc != SFE_OK) return rc;
    if (!x || n_bursts == 0) return SFE_OK;
    if (!symbols) OFDM_REFUSE("ofdm: null symbols with samples to receive");
    if (n_in >= ((size_t)1 << 31)) OFDM_REFUSE("ofdm: n_in = %zu must be below 2^31", n_in);
    if (n_bursts >= ((size_t)1 << 31)) OFDM_REFUSE("ofdm: n_bursts = %zu must be below 2^31", n_bursts);
    const int rs = check_starts("ofdm", start_base, start_step, n_bursts);
    if (rs != SFE_OK) return rs;
    const int N = sh.N;
    std::vector<double> wr(N / 2), wi(N / 2);
    for (int q = 0; q < N / 2; q++) wr[q] = std::cos(2.0 * M_PI * q / N), wi[q] = -std::sin(2.0 * M_PI * q / N);
    const long long reach = (long long)(sh.T + sh.Ns) * (N + sh.cp);
    const size_t row = (size_t)sh.Ns * sh.Nd;
    for (size_t b = 0; b < n_bursts; b++) {
        float *sym = symbols + b * 2 * row, *ch = chan ? chan + b * 2 * (size_t)N : nullptr, *rec = record ? record + b * OFDM_REC : nullptr;
        int st = OFDM_OK;
        const long long o = (long long)start_base + (long long)b * (long long)start_step + (idx ? (long long)idx[b] : 0LL);
        if (gate && !(gate[b] >= min_gate)) st = OFDM_GATED;
        else if (o < 0 || o > (long long)n_in - reach) st = OFDM_OUT_OF_RANGE;
        if (st != OFDM_OK) ofdm_fail_host(sh, sym, ch, rec);
        else st = ofdm_solve_host(sh, wr, wi, x + 2 * (size_t)o, sym, ch, rec);
        if (status) status[b] = st;
    }
    return SFE_OK;
}

int sfe_dsp_ofdm_create(int n_fft, int cp, int advance, int n_train, int n_data, const uint8_t *kind, const float *train, const float *pilot,
                        const int8_t *pilot_sign, int cfo_mode, int cfo_skip, int out_mode, float min_gate, int n_streams, int device,
                        sfe_ofdm_t *out)
{
    if (!out) return SFE_EINVAL;
    *out = nullptr;
    std::unique_ptr<Ofdm> p(new (std::nothrow) Ofdm);
    if (!p) return SFE_ENOMEM;
    int rc = ofdm_check(n_fft, cp, advance, n_train, n_data, kind, train, pilot, pilot_sign, cfo_mode, cfo_skip, out_mode, min_gate, n_streams,
                        &p->sh);
    if (rc != SFE_OK) return rc;
    CreateScope scope(device);
    if (scope.rc != SFE_OK) return scope.rc;
    p->n_streams = n_streams;
    p->device = device;
    if ((rc = p->d_tw.upload(unit_circle(n_fft, -1))) != SFE_OK || (rc = p->d_c.upload(p->sh.c)) != SFE_OK ||
        (rc = p->d_pilot.upload(p->sh.pilot)) != SFE_OK || (rc = p->d_sign.upload(p->sh.sign)) != SFE_OK ||
        (rc = p->d_bins.upload(p->sh.bins)) != SFE_OK || (rc = ofdm_prepare(p->sh.logn)) != SFE_OK)
        return rc;
    SFE_HIP(hipDeviceSynchronize());
    *out = p.release();
    return SFE_OK;
}

int sfe_dsp_ofdm_set_input_format(sfe_ofdm_t h, int fmt)
{
    // a call takes it by value when it is enqueued
    return set_format(as_ofdm(h), "ofdm_set_input_format", fmt, SFE_FMT_U8, "SFE_FMT_U8", &Ofdm::in_u8);
}

int sfe_dsp_ofdm_process_stream(sfe_ofdm_t h, const void *d_in, size_t n_in, size_t in_stride, const void *d_idx, size_t idx_stride,
                                const void *d_gate, size_t gate_stride, size_t n_bursts, int64_t start_base, int64_t start_step, void *d_out,
                                size_t out_stride, void *d_chan, void *d_rec, void *d_status, size_t status_stride, size_t *n_out,
                                sfe_stream_t stream)
{
    static const char who[] = "ofdm_process_stream";
    Ofdm *p = stream_handle(as_ofdm(h), who, n_out);
    if (!p) return SFE_EINVAL;
    const OfdmShape &sh = p->sh;
    bool go;
    int rc = check_windows(who, "n_data * Nd", (size_t)p->n_streams, p->in_u8 ? 2 : 8, d_in, n_in, in_stride, d_idx, idx_stride, d_gate,
                           gate_stride, n_bursts, start_base, start_step, d_out, out_stride, (size_t)sh.Ns * sh.Nd, d_chan, (size_t)sh.N, d_rec,
                           OFDM_REC, d_status, status_stride, &go);
    if (rc != SFE_OK || !go) return rc;
    SFE_ON_DEVICE(p->device);
    const OfdmArgs a{d_in, static_cast<const unsigned *>(d_idx), static_cast<const float *>(d_gate), p->d_tw, p->d_c, p->d_pilot, p->d_sign,
                     p->d_bins, static_cast<v2f *>(d_out), static_cast<v2f *>(d_chan), static_cast<float *>(d_rec), static_cast<int *>(d_status),
                     (long long)in_stride, (long long)idx_stride, (long long)gate_stride, (long long)out_stride, (long long)status_stride,
                     (long long)n_in, (long long)n_bursts, (long long)start_base, (long long)start_step, sh.min_gate, (float)(sh.Nd + sh.Np),
                     sh.pilot_den, sh.logn, sh.cp, sh.g, sh.T, sh.Ns, sh.Nd, sh.Np, sh.cfo, sh.q, sh.mrc};
    rc = launch_ofdm(a, p->in_u8, p->n_streams, (hipStream_t)stream);
    if (rc != SFE_OK) return rc;
    *n_out = n_bursts;
    return SFE_OK;
}

int sfe_dsp_ofdm_destroy(sfe_ofdm_t h) { return destroy_handle(as_ofdm(h)); }

}  // extern "C"
