// api_ofdmmod.hip -- the OFDM-modulator handle behind sfe_ofdmmod_t, sfe_dsp_ofdmmod_* (include/sfe_dsp.h).  Host code
// only; the kernel is in ofdmmod.hip.  Here: the checks, the tables of a shape, and sfe_dsp_ofdmmod_plan, which runs the host
// half of ofdmmod_law.h -- the header the kernel compiles too -- and so is the reference of the device's bits.
#include <cmath>

#include "host.h"
#include "block.h"
#include "ofdmmod.h"

namespace sfe {
namespace {

// a validated shape and the tables both the plan and the handle read
struct OmodShape {
    int logn = 0, N = 0, cp = 0, T = 0, Ns = 0, Nd = 0, Np = 0, order = 2, symbols = 0, tx10 = 0, F = 0;
    float amp = 0.0f, a = 0.0f;
    std::vector<omc> tw, ta, pa;        // [N] each
    std::vector<float> sign;            // [Ns]
    std::vector<int> src;               // [N]
    size_t n_in() const { return symbols ? (size_t)Ns * Nd : ((size_t)Ns * Nd * (order == 4 ? 2 : 1) + 7) / 8; }   // cf32 or bytes a burst reads
    OmodLaw law(const omc *tw_, const omc *ta_, const omc *pa_, const float *sign_, const int *src_) const
    {
        return OmodLaw{tw_, ta_, pa_, sign_, src_, logn, cp, T, Ns, Nd, order, symbols, amp, a};
    }
    OmodLaw host_law() const { return law(tw.data(), ta.data(), pa.data(), sign.data(), src.data()); }
};

#define OMOD_REFUSE(...)            \
    do {                            \
        set_error(__VA_ARGS__);     \
        return SFE_EINVAL;          \
    } while (0)

int omod_check(int n_fft, int cp, int n_train, int n_data, const uint8_t *kind, const float *train, const float *pilot, const int8_t *pilot_sign,
               float amp, int order, int in_mode, int out_fmt, OmodShape *sh)
{
    int logn = 0;
    while (logn < 31 && (1 << logn) < n_fft) logn++;
    if (n_fft < (1 << OMOD_MIN_LOGN) || n_fft > (1 << OMOD_MAX_LOGN) || (1 << logn) != n_fft)
        OMOD_REFUSE("ofdmmod: n_fft = %d must be a power of two in [%d, %d]", n_fft, 1 << OMOD_MIN_LOGN, 1 << OMOD_MAX_LOGN);
    if (cp < 0 || cp > n_fft) OMOD_REFUSE("ofdmmod: cp = %d must be in [0, n_fft = %d]", cp, n_fft);
    if (n_train < 1 || n_train > OMOD_MAX_TRAIN) OMOD_REFUSE("ofdmmod: n_train = %d must be in [1, %d]", n_train, OMOD_MAX_TRAIN);
    if (n_data < 1 || n_data > OMOD_MAX_DATA) OMOD_REFUSE("ofdmmod: n_data = %d must be in [1, %d]", n_data, OMOD_MAX_DATA);
    if ((long long)(n_train + n_data) * (n_fft + cp) >= (1LL << 31))
        OMOD_REFUSE("ofdmmod: (n_train + n_data) * (n_fft + cp) = %lld must be below 2^31", (long long)(n_train + n_data) * (n_fft + cp));
    if (!std::isfinite(amp) || !(amp > 0.0f)) OMOD_REFUSE("ofdmmod: amp must be finite and above 0");
    if (order != 2 && order != 4) OMOD_REFUSE("ofdmmod: order = %d must be 2 (BPSK) or 4 (Gray QPSK)", order);
    if (in_mode != SFE_OFDMMOD_IN_BITS && in_mode != SFE_OFDMMOD_IN_SYMBOLS)
        OMOD_REFUSE("ofdmmod: in_mode = %d must be SFE_OFDMMOD_IN_BITS (0) or SFE_OFDMMOD_IN_SYMBOLS (1)", in_mode);
    if (out_fmt != SFE_FMT_F32 && out_fmt != SFE_FMT_TX10) OMOD_REFUSE("ofdmmod: out_fmt = %d must be SFE_FMT_F32 or SFE_FMT_TX10", out_fmt);
    if (out_fmt == SFE_FMT_TX10 && (cp & 1)) OMOD_REFUSE("ofdmmod: cp = %d must be even with SFE_FMT_TX10 (a symbol is whole 5-byte groups)", cp);
    if (!kind || !train) OMOD_REFUSE("ofdmmod: null kind or train table");
    const int N = n_fft;
    sh->src.assign(N, OMOD_SRC_NULL);
    int Nd = 0, Np = 0;
    for (int k = 0; k < N; k++) {
        if (kind[k] > OMOD_KIND_PILOT) OMOD_REFUSE("ofdmmod: kind[%d] = %d must be 0 (null), 1 (data) or 2 (pilot)", k, (int)kind[k]);
        if (kind[k] == OMOD_KIND_DATA) sh->src[k] = Nd++;
        if (kind[k] == OMOD_KIND_PILOT) sh->src[k] = OMOD_SRC_PILOT, Np++;
    }
    if (Nd == 0) OMOD_REFUSE("ofdmmod: kind names no data bin");
    if (Np > 0 && !pilot) OMOD_REFUSE("ofdmmod: null pilot table with %d pilot bins", Np);
    sh->ta.assign(N, omc{0.0f, 0.0f});
    sh->pa.assign(N, omc{0.0f, 0.0f});
    for (int k = 0; k < N; k++) {
        const float tr = train[2 * k], ti = train[2 * k + 1];
        if (!std::isfinite(tr) || !std::isfinite(ti)) OMOD_REFUSE("ofdmmod: train value %d is not finite", k);
        if (pilot && (!std::isfinite(pilot[2 * k]) || !std::isfinite(pilot[2 * k + 1]))) OMOD_REFUSE("ofdmmod: pilot value %d is not finite", k);
        if (kind[k] == OMOD_KIND_NULL) continue;
        if (tr == 0.0f && ti == 0.0f) OMOD_REFUSE("ofdmmod: train value %d of a used bin is zero", k);
        sh->ta[k] = omc{amp * tr, amp * ti};
        if (kind[k] == OMOD_KIND_PILOT) {
            if (pilot[2 * k] == 0.0f && pilot[2 * k + 1] == 0.0f) OMOD_REFUSE("ofdmmod: pilot value %d of a pilot bin is zero", k);
            sh->pa[k] = omc{amp * pilot[2 * k], amp * pilot[2 * k + 1]};
        }
    }
    sh->sign.assign(n_data, 1.0f);
    for (int j = 0; pilot_sign && j < n_data; j++) {
        if (pilot_sign[j] != 1 && pilot_sign[j] != -1) OMOD_REFUSE("ofdmmod: pilot_sign[%d] = %d must be +1 or -1", j, (int)pilot_sign[j]);
        sh->sign[j] = (float)pilot_sign[j];
    }
    sh->tw.resize(N);
    om_twiddles(N, sh->tw.data());
    sh->logn = logn, sh->N = N, sh->cp = cp, sh->T = n_train, sh->Ns = n_data, sh->Nd = Nd, sh->Np = Np;
    sh->order = order, sh->symbols = in_mode == SFE_OFDMMOD_IN_SYMBOLS, sh->tx10 = out_fmt == SFE_FMT_TX10;
    sh->F = (n_train + n_data) * (N + cp);
    sh->amp = amp;
    sh->a = order == 2 ? amp : (float)((double)amp / std::sqrt(2.0));
    return SFE_OK;
}

struct Ofdmmod {
    static constexpr uint32_t MAGIC = 0x4f464d31u;   // 'OFM1'
    uint32_t magic = MAGIC;
    int device = 0;
    OmodShape sh;               // never changes after create
    DevBuf<omc> d_tw, d_ta, d_pa;
    DevBuf<float> d_sign;
    DevBuf<int> d_src;
};

Ofdmmod *as_ofdmmod(void *h) { return as_handle<Ofdmmod>(h, "OFDM-modulator"); }

inline long long ztiles_of(long long samples) { return (samples + OFDMMOD_ZTILE - 1) / OFDMMOD_ZTILE; }

}  // namespace
}  // namespace sfe

using namespace sfe;

extern "C" {

int sfe_dsp_ofdmmod_footprint(int n_fft, int *threads, int *zero_tile_samples, size_t *lds_bytes)
{
    int logn = 0;
    while (logn < 31 && (1 << logn) < n_fft) logn++;
    if (n_fft < (1 << OMOD_MIN_LOGN) || n_fft > (1 << OMOD_MAX_LOGN) || (1 << logn) != n_fft)
        OMOD_REFUSE("ofdmmod: n_fft = %d must be a power of two in [%d, %d]", n_fft, 1 << OMOD_MIN_LOGN, 1 << OMOD_MAX_LOGN);
    if (threads) *threads = ofdm_threads(logn);
    if (zero_tile_samples) *zero_tile_samples = OFDMMOD_ZTILE;
    if (lds_bytes) *lds_bytes = ofdmmod_lds_bytes(logn);
    return SFE_OK;
}

int sfe_dsp_ofdmmod_plan(int n_fft, int cp, int n_train, int n_data, const uint8_t *kind, const float *train, const float *pilot,
                         const int8_t *pilot_sign, float amp, int order, int in_mode, int out_fmt, const void *in, size_t in_stride,
                         size_t n_bursts, int64_t start_base, int64_t start_step, size_t n_out, void *out, int *n_data_bins, int *frame_len,
                         size_t *n_in)
{
    if (n_data_bins) *n_data_bins = 0;
    if (frame_len) *frame_len = 0;
    if (n_in) *n_in = 0;
    OmodShape m;
    int rc = omod_check(n_fft, cp, n_train, n_data, kind, train, pilot, pilot_sign, amp, order, in_mode, out_fmt, &m);
    if (rc != SFE_OK) return rc;
    if (n_data_bins) *n_data_bins = m.Nd;
    if (frame_len) *frame_len = m.F;
    if (n_in) *n_in = m.n_in();
    if ((rc = check_place("ofdmmod", m.F, m.tx10, m.tx10, n_bursts, start_base, start_step, n_out)) != SFE_OK) return rc;
    if (n_bursts > 0) {
        if (!in) OMOD_REFUSE("ofdmmod: null input with bursts to modulate");
        if (in_stride < m.n_in()) {
            set_error("ofdmmod: in_stride %zu < the %zu %s a burst reads", in_stride, m.n_in(), m.symbols ? "cf32 symbols" : "bytes");
            return SFE_ERANGE;
        }
    }
    if (!out || n_out == 0) return SFE_OK;
    std::vector<omc> tmp, v(m.N), w(m.N);
    omc *y = static_cast<omc *>(out);
    if (m.tx10) {
        tmp.resize(n_out);
        y = tmp.data();
    }
    for (size_t i = 0; i < n_out; i++) y[i] = omc{0.0f, 0.0f};
    const OmodLaw law = m.host_law();
    const size_t elem = m.symbols ? sizeof(omc) : 1;
    for (size_t b = 0; b < n_bursts; b++)
        om_frame_host(law, static_cast<const char *>(in) + b * in_stride * elem, v.data(), w.data(),
                      y + start_base + (int64_t)b * (n_bursts > 1 ? start_step : 0));
    if (m.tx10) om_tx10_host(y, n_out, static_cast<uint8_t *>(out));
    return SFE_OK;
}

int sfe_dsp_ofdmmod_create(int n_fft, int cp, int n_train, int n_data, const uint8_t *kind, const float *train, const float *pilot,
                           const int8_t *pilot_sign, float amp, int order, int in_mode, int out_fmt, int device, sfe_ofdmmod_t *out)
{
    if (!out) return SFE_EINVAL;
    *out = nullptr;
    std::unique_ptr<Ofdmmod> p(new (std::nothrow) Ofdmmod);
    if (!p) return SFE_ENOMEM;
    int rc = omod_check(n_fft, cp, n_train, n_data, kind, train, pilot, pilot_sign, amp, order, in_mode, out_fmt, &p->sh);
    if (rc != SFE_OK) return rc;
    CreateScope scope(device);
    if (scope.rc != SFE_OK) return scope.rc;
    p->device = device;
    const OmodShape &m = p->sh;
    if ((rc = p->d_tw.upload(m.tw)) != SFE_OK || (rc = p->d_ta.upload(m.ta)) != SFE_OK || (rc = p->d_pa.upload(m.pa)) != SFE_OK ||
        (rc = p->d_sign.upload(m.sign)) != SFE_OK || (rc = p->d_src.upload(m.src)) != SFE_OK)
        return rc;
    *out = p.release();
    return SFE_OK;
}

int sfe_dsp_ofdmmod_process_stream(sfe_ofdmmod_t h, const void *d_in, size_t in_stride, size_t n_bursts, int64_t start_base, int64_t start_step,
                                   void *d_out, size_t n_out, size_t *n_written, sfe_stream_t stream)
{
    static const char who[] = "ofdmmod_process_stream";
    Ofdmmod *p = stream_handle(as_ofdmmod(h), who, n_written, "n_written");
    if (!p) return SFE_EINVAL;
    const OmodShape &m = p->sh;
    const FrameNouns nouns{"the ", m.symbols ? " cf32 symbols a burst reads" : " bytes a burst reads", "input's",
                           "cf32 input and output 8 B; TX10 output and coded bytes need none"};
    bool go;
    int rc = check_frames(who, nouns, m.F, m.tx10, m.tx10, d_in, in_stride, m.n_in(), m.symbols ? sizeof(omc) : 1, n_bursts, start_base,
                          start_step, d_out, n_out, &go);
    if (rc != SFE_OK || !go) return rc;
    const long long nb = (long long)n_bursts, step = nb > 1 ? start_step : 0;
    const long long last_end = nb ? start_base + (nb - 1) * step + m.F : 0;
    OfdmmodArgs a{};
    a.n_lead = ztiles_of(nb ? start_base : (long long)n_out);
    a.gap_tiles = nb > 1 ? ztiles_of(start_step - m.F) : 0;
    const __int128 n_wg = (__int128)a.n_lead + (__int128)nb * (m.T + m.Ns + a.gap_tiles) + (nb ? ztiles_of((long long)n_out - last_end) : 0);
    if (n_wg >= ((__int128)1 << 31)) {
        set_error("ofdmmod_process_stream: the call's workgroups (a symbol, or %d samples of zeros, each) must number below 2^31", OFDMMOD_ZTILE);
        return SFE_EINVAL;
    }
    SFE_ON_DEVICE(p->device);
    a.law = m.law(p->d_tw, p->d_ta, p->d_pa, p->d_sign, p->d_src);
    a.in = d_in, a.out = d_out;
    a.in_stride = (long long)in_stride, a.start_base = nb ? start_base : 0, a.start_step = step;
    a.n_out = (long long)n_out, a.n_bursts = nb;
    a.F = m.F, a.tx10 = m.tx10;
    if ((rc = launch_ofdmmod(a, (long long)n_wg, (hipStream_t)stream)) != SFE_OK) return rc;
    *n_written = n_out;
    return SFE_OK;
}

int sfe_dsp_ofdmmod_destroy(sfe_ofdmmod_t h) { return destroy_handle(as_ofdmmod(h)); }

}  // extern "C"
