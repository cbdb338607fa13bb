// api_fsk.hip -- the 2-(G)FSK modem handle behind sfe_fsk_t, sfe_dsp_fsk_* (include/sfe_dsp.h).  Host code only; the
// kernels are in fsk.hip.  Here: the checks, the tables of a shape (the integer pulse and its running sum, the expected
// response of the preamble), and sfe_dsp_fsk_plan, which runs the host half of fsk_law.h -- the header the kernels compile
// too -- and so is the reference of the device's bits.
#include <cmath>
#include <cstring>

#include "host.h"
#include "block.h"
#include "fsk.h"
#include "ofdmmod_law.h"

namespace sfe {
namespace {

#define FSK_REFUSE(...)             \
    do {                            \
        set_error(__VA_ARGS__);     \
        return SFE_EINVAL;          \
    } while (0)

// a validated shape and its tables
struct FskShape {
    int sps = 0, n_taps = 0, Q = 0, Lp = 0, n_bits = 0, N = 0, F = 0, n_mf = 0, delay = 0, R = 0, tx10 = 0;
    float amp = 0.0f, scale = 0.0f, min_gate = 0.0f, se = 0.0f, see = 0.0f, den = 0.0f;
    uint32_t Gsum = 0;
    std::vector<uint32_t> C;            // [n_taps + 1]
    std::vector<uint8_t> pre, packed;   // [Lp] 0/1; [ceil(Lp / 8)] MSB-first
    std::vector<float> mf, e;           // [n_mf]; [Lp]
    size_t nbytes() const { return ((size_t)n_bits + 7) / 8; }
};

int fsk_check(int sps, const float *pulse, int n_taps, float h, float amp, const uint8_t *pre, int n_pre, int n_bits, const float *mf, int n_mf,
              int delay, int range, float scale, float min_gate, int out_fmt, int n_streams, FskShape *sh)
{
    if (sps < FSK_MIN_SPS || sps > FSK_MAX_SPS) FSK_REFUSE("fsk: sps = %d must be in [%d, %d]", sps, FSK_MIN_SPS, FSK_MAX_SPS);
    if (n_taps < 1 || n_taps > FSK_MAX_ARM * sps || !pulse)
        FSK_REFUSE("fsk: n_taps = %d must be in [1, %d sps = %d], with a pulse", n_taps, FSK_MAX_ARM, FSK_MAX_ARM * sps);
    for (int j = 0; j < n_taps; j++)
        if (!std::isfinite(pulse[j])) FSK_REFUSE("fsk: pulse value %d is not finite", j);
    if (!std::isfinite(h) || !(h > 0.0f)) FSK_REFUSE("fsk: the modulation index h must be finite and above 0");
    if (!std::isfinite(amp) || !(amp > 0.0f)) FSK_REFUSE("fsk: amp must be finite and above 0");
    if (n_pre < 2 || n_pre > FSK_MAX_PRE || !pre) FSK_REFUSE("fsk: n_pre = %d must be in [2, %d], with preamble bits", n_pre, FSK_MAX_PRE);
    for (int k = 0; k < n_pre; k++)
        if (pre[k] > 1) FSK_REFUSE("fsk: preamble bit %d is %u, not 0 or 1", k, pre[k]);
    if (n_bits < 1 || n_bits > FSK_MAX_BITS) FSK_REFUSE("fsk: n_bits = %d must be in [1, %d]", n_bits, FSK_MAX_BITS);
    if (n_mf < 1 || n_mf > FSK_MAX_MF || !mf) FSK_REFUSE("fsk: n_mf = %d must be in [1, %d], with a matched filter", n_mf, FSK_MAX_MF);
    double sm = 0.0;
    for (int j = 0; j < n_mf; j++) {
        if (!std::isfinite(mf[j])) FSK_REFUSE("fsk: matched-filter value %d is not finite", j);
        sm += (double)mf[j];
    }
    if (!(sm > 0.0)) FSK_REFUSE("fsk: the matched filter's sum must be above 0");
    if (delay < 1 || delay > FSK_MAX_DELAY) FSK_REFUSE("fsk: delay = %d must be in [1, 2^20]", delay);
    if (range < 0 || range > FSK_MAX_RANGE) FSK_REFUSE("fsk: range = %d must be in [0, %d]", range, FSK_MAX_RANGE);
    if (!std::isfinite(scale) || !(scale > 0.0f)) FSK_REFUSE("fsk: scale must be finite and above 0");
    if (!std::isfinite(min_gate)) FSK_REFUSE("fsk: min_gate must be finite");
    if (n_streams < 1) FSK_REFUSE("fsk: n_streams = %d must be at least 1", n_streams);
    if (out_fmt != SFE_FMT_F32 && out_fmt != SFE_FMT_TX10) FSK_REFUSE("fsk: out_fmt = %d must be SFE_FMT_F32 or SFE_FMT_TX10", out_fmt);

    // ---- the integer pulse: G[j] = rint(h g[j] 2^31), formed in float64 and rounded once
    std::vector<long long> G(n_taps);
    long long gsum = 0;
    for (int j = 0; j < n_taps; j++) {
        const double v = std::rint((double)h * (double)pulse[j] * 2147483648.0);
        if (!(std::fabs(v) < 1073741824.0)) FSK_REFUSE("fsk: h * pulse[%d] is a quarter turn a sample or more", j);
        G[j] = (long long)v;
        gsum += G[j];
    }
    if (gsum <= 0) FSK_REFUSE("fsk: the integer pulse's sum must be above 0");
    for (int r = 0; r < sps; r++) {
        long long a = 0;
        for (int j = r; j < n_taps; j += sps) a += G[j] < 0 ? -G[j] : G[j];
        if (a >= (1LL << 30))
            FSK_REFUSE("fsk: the pulse's values %d mod sps sum to a quarter turn a sample or more (the discriminator needs the room)", r);
    }
    sh->sps = sps, sh->n_taps = n_taps, sh->Q = (n_taps + sps - 1) / sps, sh->Lp = n_pre, sh->n_bits = n_bits, sh->N = n_pre + n_bits;
    sh->F = (sh->N + sh->Q - 1) * sps + 1;
    sh->n_mf = n_mf, sh->delay = delay, sh->R = range, sh->tx10 = out_fmt == SFE_FMT_TX10;
    sh->amp = amp, sh->scale = scale, sh->min_gate = min_gate;
    sh->C.assign((size_t)n_taps + 1, 0u);
    for (int j = 0; j < n_taps; j++) sh->C[j + 1] = sh->C[j] + (uint32_t)G[j];
    sh->Gsum = sh->C[n_taps];
    sh->pre.assign(pre, pre + n_pre);
    sh->packed.assign(((size_t)n_pre + 7) / 8, 0);
    for (int k = 0; k < n_pre; k++) sh->packed[k >> 3] |= (uint8_t)(pre[k] << (7 - (k & 7)));
    sh->mf.assign(mf, mf + n_mf);

    // ---- the expected response of the preamble, in float64 from the integer pulse, data symbols taken as 0
    const long long nd = (long long)(n_pre - 1) * sps + n_taps;
    std::vector<long long> D((size_t)nd, 0);
    for (int k = 0; k < n_pre; k++)
        for (int j = 0; j < n_taps; j++) D[(size_t)k * sps + j] += pre[k] ? -G[j] : G[j];
    const double U = (double)gsum / (double)sps * sm;
    sh->e.resize(n_pre);
    double se = 0.0, see = 0.0;
    for (int k = 0; k < n_pre; k++) {
        double acc = 0.0;
        for (int j = 0; j < n_mf; j++) {
            const long long i = (long long)delay + (long long)k * sps + j - 1;
            if (i < nd) acc += (double)mf[j] * (double)D[(size_t)i];
        }
        sh->e[k] = (float)(acc / U);
        se += (double)sh->e[k];
        see += (double)sh->e[k] * (double)sh->e[k];
    }
    sh->se = (float)se, sh->see = (float)see, sh->den = (float)((double)n_pre * see - se * se);
    if (!(sh->den > 0.0f) || !std::isfinite(sh->den))
        FSK_REFUSE("fsk: the preamble's expected response has no spread (den = n_pre * sum e^2 - (sum e)^2 is not above 0)");
    return SFE_OK;
}

// one frame by the law: F samples into y
void fsk_frame_host(const FskShape &m, const uint8_t *row, v2f *y)
{
    std::vector<int> cum((size_t)m.N + 1, 0);       // cum[k]: the sum of the levels of the symbols before k
    auto lev = [&](int k) { return 1 - 2 * (int)(k < m.Lp ? m.pre[k] : fsk_bit(row, k - m.Lp)); };
    for (int k = 0; k < m.N; k++) cum[k + 1] = cum[k] + lev(k);
    for (int i = 0; i < m.F; i++) {
        const int kp = fsk_passed(i, m.sps, m.n_taps, m.N);
        const FskC s = fsk_mod_sample(fsk_phase(i, m.sps, m.N, m.Gsum, cum[kp], kp, m.C.data(), lev), m.amp);
        y[i] = v2f{s.r, s.i};
    }
}

void fsk_fill_host(const FskShape &m, float *soft, uint8_t *bits, float *rec)
{
    for (int t = 0; t < m.n_bits; t++) soft[t] = 0.0f;
    if (bits) std::memset(bits, 0, m.nbytes());
    if (rec)
        for (int i = 0; i < FSK_REC; i++) rec[i] = i < 4 ? std::nanf("") : 0.0f;
}

// one burst by the law; x0: sample 0 of the burst (its reach is inside the stream).  Returns the status.
int fsk_burst_host(const FskShape &m, const float *x0, float *soft, uint8_t *bits, float *rec)
{
    auto at = [&](long long n) { return PolarC{x0[2 * n], x0[2 * n + 1]}; };
    const long long lo = (long long)m.delay - m.R - 1, hi = (long long)m.delay + m.R + (long long)(m.N - 1) * m.sps + m.n_mf;
    for (long long i = 2 * lo; i < 2 * hi; i++)
        if (!std::isfinite(x0[i])) return fsk_fill_host(m, soft, bits, rec), FSK_NO_ESTIMATE;
    const int Lp = m.Lp, Lp2 = fsk_pow2(Lp);
    std::vector<float> t1((size_t)Lp2), te((size_t)Lp2);
    bool have = false;
    float best = 0.0f, best_S1 = 0.0f;
    int tau = 0;
    for (int c = -m.R; c <= m.R; c++) {
        for (int k = 0; k < Lp2; k++) {
            const float u = k < Lp ? fsk_u((long long)m.delay + c + (long long)k * m.sps, m.n_mf, m.mf.data(), at) : 0.0f;
            t1[k] = u;
            te[k] = k < Lp ? m.e[k] * u : 0.0f;
        }
        const float S1 = fsk_tree(t1.data(), Lp2), n = fsk_num(Lp, fsk_tree(te.data(), Lp2), m.se, S1);
        if (n == n && (!have || n > best)) have = true, best = n, best_S1 = S1, tau = c;
    }
    if (!have) return fsk_fill_host(m, soft, bits, rec), FSK_NO_ESTIMATE;
    const FskFit fit = fsk_fit(Lp, best, m.den, m.se, best_S1);
    if (!fsk_fit_ok(fit.dev)) return fsk_fill_host(m, soft, bits, rec), FSK_NO_ESTIMATE;
    for (int k = 0; k < Lp2; k++)
        t1[k] = k < Lp ? fsk_resid_term(fsk_u((long long)m.delay + tau + (long long)k * m.sps, m.n_mf, m.mf.data(), at), m.e[k], fit.dev, fit.dc) : 0.0f;
    const float q = fsk_quality(fsk_tree(t1.data(), Lp2), fit.dev, m.see);
    if (bits) std::memset(bits, 0, m.nbytes());
    for (int t = 0; t < m.n_bits; t++) {
        const float r = fsk_soft(fsk_u((long long)m.delay + tau + (long long)(Lp + t) * m.sps, m.n_mf, m.mf.data(), at), fit.dc, fit.dev, m.scale);
        soft[t] = r;
        if (bits && r < 0.0f) bits[t >> 3] |= (uint8_t)(0x80u >> (t & 7));
    }
    if (rec) {
        rec[0] = (float)tau, rec[1] = fit.f, rec[2] = fit.dev, rec[3] = q;
        rec[4] = rec[5] = rec[6] = rec[7] = 0.0f;
    }
    return FSK_OK;
}

struct Fsk {
    static constexpr uint32_t MAGIC = 0x46534b31u;   // 'FSK1'
    uint32_t magic = MAGIC;
    int device = 0, n_streams = 1, in_u8 = 0;
    FskShape shape;             // never changes after create
    DevBuf<uint32_t> d_C;
    DevBuf<uint8_t> d_pre;
    DevBuf<float> d_mf, d_e;
};

Fsk *as_fsk(void *h) { return as_handle<Fsk>(h, "FSK-modem"); }

inline long long tiles_of(long long samples) { return (samples + FSK_TILE - 1) / FSK_TILE; }

}  // namespace
}  // namespace sfe

using namespace sfe;

extern "C" {

int sfe_dsp_fsk_plan(int sps, const float *pulse, int n_taps, float h, float amp, const uint8_t *pre, int n_pre, int n_bits, const float *mf,
                     int n_mf, int delay, int range, float scale, float min_gate, int out_fmt, int direction, const void *in, size_t in_len,
                     const uint32_t *idx, const float *gate, size_t n_bursts, int64_t start_base, int64_t start_step, void *out, size_t n_out,
                     uint8_t *bits, float *record, int *status, int *n_sym, int *frame_len, float *e, float *den)
{
    if (n_sym) *n_sym = 0;
    if (frame_len) *frame_len = 0;
    if (den) *den = 0.0f;
    FskShape m;
    int rc = fsk_check(sps, pulse, n_taps, h, amp, pre, n_pre, n_bits, mf, n_mf, delay, range, scale, min_gate, out_fmt, 1, &m);
    if (rc != SFE_OK) return rc;
    if (n_sym) *n_sym = m.N;
    if (frame_len) *frame_len = m.F;
    if (den) *den = m.den;
    if (e) std::memcpy(e, m.e.data(), (size_t)m.Lp * sizeof(float));
    if (direction != SFE_FSK_MOD && direction != SFE_FSK_DEMOD) FSK_REFUSE("fsk: direction = %d must be SFE_FSK_MOD (0) or SFE_FSK_DEMOD (1)", direction);

    if (direction == SFE_FSK_MOD) {
        if ((rc = check_place("fsk", m.F, m.tx10, false, n_bursts, start_base, start_step, n_out)) != SFE_OK) return rc;
        if (n_bursts > 0) {
            if (!in) FSK_REFUSE("fsk: null bytes with bursts to modulate");
            if (in_len < m.nbytes()) {
                set_error("fsk: in_stride %zu < ceil(n_bits / 8) = %zu", in_len, m.nbytes());
                return SFE_ERANGE;
            }
        }
        if (!out || n_out == 0) return SFE_OK;
        std::vector<v2f> tmp;
        v2f *y = static_cast<v2f *>(out);
        if (m.tx10) {
            tmp.resize(n_out);
            y = tmp.data();
        }
        for (size_t i = 0; i < n_out; i++) y[i] = v2f{0.0f, 0.0f};
        for (size_t b = 0; b < n_bursts; b++)
            fsk_frame_host(m, static_cast<const uint8_t *>(in) + b * in_len, y + start_base + (int64_t)b * (n_bursts > 1 ? start_step : 0));
        // the wire format's law is ofdmmod_law.h's, as for mod: the same quantiser, the same groups
        static_assert(sizeof(omc) == sizeof(v2f) && alignof(omc) == alignof(v2f), "om_tx10_host reads v2f samples");
        if (m.tx10) om_tx10_host(reinterpret_cast<const omc *>(y), n_out, static_cast<uint8_t *>(out));
        return SFE_OK;
    }

    if (!in || n_bursts == 0) return SFE_OK;
    if (!out) FSK_REFUSE("fsk: null soft values with samples to demodulate");
    if (in_len >= ((size_t)1 << 31) || n_bursts >= ((size_t)1 << 31)) FSK_REFUSE("fsk: n_in = %zu and n_bursts = %zu must be below 2^31", in_len, n_bursts);
    if ((rc = check_starts("fsk", start_base, start_step, n_bursts)) != SFE_OK) return rc;
    const float *x = static_cast<const float *>(in);
    for (size_t b = 0; b < n_bursts; b++) {
        float *soft = static_cast<float *>(out) + b * (size_t)m.n_bits, *rec = record ? record + b * FSK_REC : nullptr;
        uint8_t *by = bits ? bits + b * m.nbytes() : nullptr;
        int st = FSK_OK;
        const long long o = (long long)start_base + (long long)b * (long long)start_step + (idx ? (long long)idx[b] : 0LL);
        const long long lo = o + m.delay - m.R - 1, hi = o + m.delay + m.R + (long long)(m.N - 1) * m.sps + m.n_mf;
        if (gate && !(gate[b] >= m.min_gate)) st = FSK_GATED;
        else if (lo < 0 || hi > (long long)in_len) st = FSK_OUT_OF_RANGE;
        if (st != FSK_OK) fsk_fill_host(m, soft, by, rec);
        else st = fsk_burst_host(m, x + 2 * o, soft, by, rec);
        if (status) status[b] = st;
    }
    return SFE_OK;
}

int sfe_dsp_fsk_create(int sps, const float *pulse, int n_taps, float h, float amp, const uint8_t *pre, int n_pre, int n_bits, const float *mf,
                       int n_mf, int delay, int range, float scale, float min_gate, int out_fmt, int n_streams, int device, sfe_fsk_t *out)
{
    if (!out) return SFE_EINVAL;
    *out = nullptr;
    std::unique_ptr<Fsk> p(new (std::nothrow) Fsk);
    if (!p) return SFE_ENOMEM;
    int rc = fsk_check(sps, pulse, n_taps, h, amp, pre, n_pre, n_bits, mf, n_mf, delay, range, scale, min_gate, out_fmt, n_streams, &p->shape);
    if (rc != SFE_OK) return rc;
    CreateScope scope(device);
    if (scope.rc != SFE_OK) return scope.rc;
    p->device = device, p->n_streams = n_streams;
    const FskShape &m = p->shape;
    if ((rc = p->d_C.upload(m.C)) != SFE_OK || (rc = p->d_pre.upload(m.packed)) != SFE_OK || (rc = p->d_mf.upload(m.mf)) != SFE_OK ||
        (rc = p->d_e.upload(m.e)) != SFE_OK)
        return rc;
    *out = p.release();
    return SFE_OK;
}

int sfe_dsp_fsk_set_input_format(sfe_fsk_t h, int fmt)
{
    return set_format(as_fsk(h), "fsk_set_input_format", fmt, SFE_FMT_U8, "SFE_FMT_U8", &Fsk::in_u8);
}

int sfe_dsp_fsk_mod_stream(sfe_fsk_t h, const void *d_bytes, size_t in_stride, size_t n_bursts, int64_t start_base, int64_t start_step,
                           void *d_out, size_t n_out, size_t *n_written, sfe_stream_t stream)
{
    static const char who[] = "fsk_mod_stream";
    Fsk *p = stream_handle(as_fsk(h), who, n_written, "n_written");
    if (!p) return SFE_EINVAL;
    const FskShape &m = p->shape;
    static const FrameNouns nouns{"ceil(n_bits / 8) = ", "", "payloads'", "cf32 output 8 B; TX10 output and payload bytes need none"};
    bool go;
    int rc = check_frames(who, nouns, m.F, m.tx10, false, d_bytes, in_stride, m.nbytes(), 1, n_bursts, start_base, start_step, d_out, n_out, &go);
    if (rc != SFE_OK || !go) return rc;
    const long long nb = (long long)n_bursts;
    const long long last_end = nb ? start_base + (nb - 1) * (nb > 1 ? start_step : 0) + m.F : 0;
    FskModArgs a{};
    a.n_lead = tiles_of(nb ? start_base : (long long)n_out);
    a.tiles_per_slot = nb ? tiles_of(nb > 1 ? start_step : m.F) : 0;
    const __int128 n_tiles = (__int128)a.n_lead + (__int128)nb * a.tiles_per_slot + (nb ? tiles_of((long long)n_out - last_end) : 0);
    if (n_tiles >= ((__int128)1 << 31)) {
        set_error("fsk_mod_stream: the call's %d-sample tiles must number below 2^31", FSK_TILE);
        return SFE_EINVAL;
    }
    SFE_ON_DEVICE(p->device);
    a.bytes = static_cast<const uint8_t *>(d_bytes), a.out = d_out, a.C = p->d_C, a.pre = p->d_pre;
    a.in_stride = (long long)in_stride, a.start_base = nb ? start_base : 0, a.start_step = nb > 1 ? start_step : 0;
    a.n_out = (long long)n_out, a.n_bursts = nb;
    a.Gsum = m.Gsum, a.Lp = m.Lp, a.N = m.N, a.sps = m.sps, a.n_taps = m.n_taps, a.F = m.F, a.amp = m.amp;
    if ((rc = launch_fsk_mod(a, m.tx10, (long long)n_tiles, (hipStream_t)stream)) != SFE_OK) return rc;
    *n_written = n_out;
    return SFE_OK;
}

int sfe_dsp_fsk_demod_stream(sfe_fsk_t h, const void *d_in, size_t n_in, size_t in_stride, const void *d_idx, size_t idx_stride,
                             const void *d_gate, size_t gate_stride, size_t n_bursts, int64_t start_base, int64_t start_step, void *d_soft,
                             size_t soft_stride, void *d_bits, size_t bits_stride, void *d_rec, void *d_status, size_t status_stride,
                             size_t *n_out, sfe_stream_t stream)
{
    static const char who[] = "fsk_demod_stream";
    Fsk *p = stream_handle(as_fsk(h), who, n_out);
    if (!p) return SFE_EINVAL;
    const FskShape &m = p->shape;
    const size_t S = (size_t)p->n_streams, isz = p->in_u8 ? 2 : 8;
    int rc = refuse_2_31(who, n_in);
    if (rc != SFE_OK) return rc;
    if (n_bursts >= ((size_t)1 << 31) / S) {
        set_error("%s: n_streams * n_bursts = %zu * %zu must be below 2^31 per call", who, S, n_bursts);
        return SFE_EINVAL;
    }
    if (n_bursts == 0) return SFE_OK;
    if ((rc = refuse_null(who, {d_in, d_soft})) != SFE_OK) return rc;
    if (soft_stride < (size_t)m.n_bits || (d_bits && bits_stride < m.nbytes()) || (d_status && status_stride < n_bursts)) {
        set_error("%s: soft_stride %zu < n_bits = %d, bits_stride %zu < ceil(n_bits / 8) = %zu or status_stride %zu < n_bursts = %zu", who,
                  soft_stride, m.n_bits, bits_stride, m.nbytes(), status_stride, n_bursts);
        return SFE_ERANGE;
    }
    if ((rc = refuse_short_streams(who, S, in_stride, n_in)) != SFE_OK || (rc = check_starts(who, start_base, start_step, n_bursts)) != SFE_OK) return rc;
    const size_t rows = S * n_bursts;
    size_t in_b = 0, ix_b = 0, ga_b = 0, so_b = 0, bi_b = 0, st_b = 0;
    if (!span_bytes(S - 1, in_stride, n_in, isz, &in_b) || (d_idx && !span_bytes(S - 1, idx_stride, n_bursts, 4, &ix_b)) ||
        (d_gate && !span_bytes(S - 1, gate_stride, n_bursts, 4, &ga_b)) || !span_bytes(rows - 1, soft_stride, (size_t)m.n_bits, 4, &so_b) ||
        (d_bits && !span_bytes(rows - 1, bits_stride, m.nbytes(), 1, &bi_b)) || (d_status && !span_bytes(S - 1, status_stride, n_bursts, 4, &st_b)))
        return refuse_2_62(who);
    const Span in{d_in, in_b, isz}, ix{d_idx, ix_b, 4}, ga{d_gate, ga_b, 4}, so{d_soft, so_b, 4}, bi{d_bits, bi_b, 1};
    const Span re{d_rec, d_rec ? rows * FSK_REC * 4 : 0, 4}, st{d_status, st_b, 4};
    if ((rc = refuse_misaligned(who, "cf32 8 B, u8 (I,Q) pairs 2 B, indices, gates, soft values, records and statuses 4 B", {in, ix, ga, so, re, st})) != SFE_OK ||
        (rc = refuse_overlap(who, in, {so, bi, re, st})) != SFE_OK || (rc = refuse_overlap(who, ix, {so, bi, re, st})) != SFE_OK ||
        (rc = refuse_overlap(who, ga, {so, bi, re, st})) != SFE_OK || (rc = refuse_outputs_overlap(who, {so, bi, re, st})) != SFE_OK)
        return rc;
    SFE_ON_DEVICE(p->device);
    FskDemodArgs a{};
    a.in = d_in, a.idx = static_cast<const unsigned *>(d_idx), a.gate = static_cast<const float *>(d_gate), a.mf = p->d_mf, a.e = p->d_e;
    a.soft = static_cast<float *>(d_soft), a.bits = static_cast<uint8_t *>(d_bits), a.rec = static_cast<float *>(d_rec);
    a.status = static_cast<int *>(d_status);
    a.in_stride = (long long)in_stride, a.idx_stride = (long long)idx_stride, a.gate_stride = (long long)gate_stride;
    a.soft_stride = (long long)soft_stride, a.bits_stride = (long long)bits_stride, a.status_stride = (long long)status_stride;
    a.n_in = (long long)n_in, a.n_bursts = (long long)n_bursts, a.start_base = start_base, a.start_step = start_step;
    a.se = m.se, a.see = m.see, a.den = m.den, a.scale = m.scale, a.min_gate = m.min_gate;
    a.sps = m.sps, a.Lp = m.Lp, a.N = m.N, a.n_mf = m.n_mf, a.delay = m.delay, a.R = m.R;
    if ((rc = launch_fsk_demod(a, p->in_u8, p->n_streams, (hipStream_t)stream)) != SFE_OK) return rc;
    *n_out = n_bursts;
    return SFE_OK;
}

int sfe_dsp_fsk_destroy(sfe_fsk_t h) { return destroy_handle(as_fsk(h)); }

}  // extern "C"
