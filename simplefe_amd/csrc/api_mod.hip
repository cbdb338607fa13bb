// api_mod.hip -- the burst-modulator handle behind sfe_mod_t, sfe_dsp_mod_* (include/sfe_dsp.h).  Host code only; the
// kernel is in mod.hip.  Here: the checks, and the host twin of the kernel's law (sfe_dsp_mod_plan: the reference of the
// device's bits -- a sequential encoder, the symbol map, and the same fmaf chains in the same order, every skipped term
// skipped literally).
#include <cmath>
#include <cstring>

#include "host.h"
#include "block.h"
#include "mod.h"
#include "ofdmmod_law.h"
#include "vit_code.h"

namespace sfe {
namespace {

// a validated shape: code, mapping, preamble, pulse, output format
struct ModShape {
    VitCode code;               // n = 0: uncoded (only n_info and n_soft mean anything)
    int order = 2, Lp = 0, n_data = 0, N = 0, sps = 1, n_taps = 0, Q = 0, F = 0, tx10 = 0;
    float amp = 0.0f, a = 0.0f; // a: a data symbol's component
    std::vector<float> taps;
    std::vector<v2f> pre;       // amp p[k], one float32 product per component
    uint8_t pos[MOD_TABLE] = {};
    size_t nbytes() const { return ((size_t)code.n_info + 7) / 8; }
};

int mod_check(int K, int n_gen, const uint32_t *gen, const uint8_t *keep, int P, int terminated, int n_info, int order, const float *preamble,
              int n_pre, int sps, const float *taps, int n_taps, float amp, int out_fmt, ModShape *m)
{
    VitCode &c = m->code;
    if (n_gen == 0) {
        if (n_info < 1 || n_info > VIT_MAX_INFO) {
            set_error("mod: n_info = %d must be in [1, %d]", n_info, VIT_MAX_INFO);
            return SFE_EINVAL;
        }
        c = VitCode{};
        c.n_info = c.T = c.n_soft = n_info;
    } else {
        const int rc = vit_check_code("mod", K, n_gen, gen, keep, P, terminated, n_info < 0 ? 0 : (size_t)n_info, &c);
        if (rc != SFE_OK) return rc;
        int i = 0;
        for (int tp = 0; tp < c.P; tp++)
            for (int j = 0; j < c.n; j++)
                if (c.kept(tp, j)) m->pos[i++] = (uint8_t)(tp << 2 | j);
    }
    if (order != 2 && order != 4) {
        set_error("mod: order = %d must be 2 (BPSK) or 4 (Gray QPSK)", order);
        return SFE_EINVAL;
    }
    if (!std::isfinite(amp) || !(amp > 0.0f)) {
        set_error("mod: amp must be finite and above 0");
        return SFE_EINVAL;
    }
    if (n_pre < 0 || n_pre > MOD_MAX_PRE || (n_pre > 0 && !preamble)) {
        set_error("mod: n_pre = %d must be in [0, %d], with a preamble where it is not 0", n_pre, MOD_MAX_PRE);
        return SFE_EINVAL;
    }
    for (int i = 0; i < 2 * n_pre; i++)
        if (!std::isfinite(preamble[i])) {
            set_error("mod: preamble symbol %d is not finite", i / 2);
            return SFE_EINVAL;
        }
    if (sps < 1 || sps > MOD_MAX_SPS) {
        set_error("mod: sps = %d must be in [1, %d]", sps, MOD_MAX_SPS);
        return SFE_EINVAL;
    }
    if (n_taps < 1 || n_taps > MOD_MAX_ARM * sps || !taps) {
        set_error("mod: n_taps = %d must be in [1, %d sps = %d], with taps", n_taps, MOD_MAX_ARM, MOD_MAX_ARM * sps);
        return SFE_EINVAL;
    }
    for (int i = 0; i < n_taps; i++)
        if (!std::isfinite(taps[i])) {
            set_error("mod: tap %d is not finite", i);
            return SFE_EINVAL;
        }
    if (out_fmt != SFE_FMT_F32 && out_fmt != SFE_FMT_TX10) {
        set_error("mod: out_fmt = %d must be SFE_FMT_F32 or SFE_FMT_TX10", out_fmt);
        return SFE_EINVAL;
    }
    m->order = order, m->Lp = n_pre, m->sps = sps, m->n_taps = n_taps, m->tx10 = out_fmt == SFE_FMT_TX10;
    m->amp = amp;
    m->a = order == 2 ? amp : (float)((double)amp / std::sqrt(2.0));
    m->n_data = order == 2 ? c.n_soft : (c.n_soft + 1) / 2;
    m->N = n_pre + m->n_data;
    m->Q = (n_taps + sps - 1) / sps;
    m->F = (m->N + m->Q - 1) * sps;
    m->taps.assign(taps, taps + n_taps);
    m->pre.resize(n_pre);
    for (int k = 0; k < n_pre; k++) m->pre[k] = v2f{amp * preamble[2 * k], amp * preamble[2 * k + 1]};
    return SFE_OK;
}

// the symbols of one burst by the law: a sequential encoder, then the map
void mod_symbols_host(const ModShape &m, const uint8_t *row, std::vector<v2f> &s)
{
    const VitCode &c = m.code;
    std::vector<uint8_t> coded;
    coded.reserve((size_t)c.n_soft + 1);
    auto bit = [&](int t) { return (unsigned)(row[t >> 3] >> (7 - (t & 7))) & 1u; };
    if (c.n == 0) {
        for (int t = 0; t < c.n_info; t++) coded.push_back((uint8_t)bit(t));
    } else {
        unsigned reg = 0;
        for (int t = 0; t < c.T; t++) {
            reg = ((reg << 1) | (t < c.n_info ? bit(t) : 0u)) & ((1u << c.K) - 1u);
            const unsigned l = c.label(reg);
            for (int j = 0; j < c.n; j++)
                if (c.kept(t % c.P, j)) coded.push_back((uint8_t)((l >> j) & 1u));
        }
    }
    if (coded.size() & 1) coded.push_back(0);                   // the pad of an odd n_soft under QPSK
    s.assign(m.pre.begin(), m.pre.end());
    for (int i = 0; i < m.n_data; i++) {
        if (m.order == 2) s.push_back(v2f{coded[i] ? -m.a : m.a, 0.0f});
        else s.push_back(v2f{coded[2 * i] ? -m.a : m.a, coded[2 * i + 1] ? -m.a : m.a});
    }
}

// the frame of one burst: F samples into y
void mod_frame_host(const ModShape &m, const std::vector<v2f> &s, v2f *y)
{
    for (int k = 0; k < m.N + m.Q - 1; k++)
        for (int r = 0; r < m.sps; r++) {
            float ax = 0.0f, ay = 0.0f;
            for (int q = 0; q < m.Q; q++) {
                if (k - q < 0 || k - q >= m.N || q * m.sps + r >= m.n_taps) continue;
                const float h = m.taps[q * m.sps + r];
                ax = std::fmaf(h, s[k - q].x, ax);
                ay = std::fmaf(h, s[k - q].y, ay);
            }
            y[(size_t)k * m.sps + r] = v2f{ax, ay};
        }
}

struct Mod {
    static constexpr uint32_t MAGIC = 0x4D4F4431u;   // 'MOD1'
    uint32_t magic = MAGIC;
    int device = 0;
    ModShape shape;             // never changes after create
    DevBuf<float> d_taps;
    DevBuf<v2f> d_pre;
};

Mod *as_mod(void *h) { return as_handle<Mod>(h, "burst-modulator"); }

inline long long tiles_of(long long samples) { return (samples + MOD_TILE - 1) / MOD_TILE; }

}  // namespace
}  // namespace sfe

using namespace sfe;

extern "C" {

int sfe_dsp_mod_footprint(int *tile_samples, size_t *lds_bytes)
{
    if (tile_samples) *tile_samples = MOD_TILE;
    if (lds_bytes) *lds_bytes = MOD_LDS_BYTES;
    return SFE_OK;
}

int sfe_dsp_mod_plan(int K, int n_gen, const uint32_t *gen, const uint8_t *keep, int P, int terminated, int n_info, int order,
                     const float *preamble, int n_pre, int sps, const float *taps, int n_taps, float amp, int out_fmt,
                     const uint8_t *bytes, size_t in_stride, size_t n_bursts, int64_t start_base, int64_t start_step, size_t n_out,
                     void *out, int *n_sym, int *frame_len, size_t *n_soft)
{
    if (n_sym) *n_sym = 0;
    if (frame_len) *frame_len = 0;
    if (n_soft) *n_soft = 0;
    ModShape m;
    int rc = mod_check(K, n_gen, gen, keep, P, terminated, n_info, order, preamble, n_pre, sps, taps, n_taps, amp, out_fmt, &m);
    if (rc != SFE_OK) return rc;
    if (n_sym) *n_sym = m.N;
    if (frame_len) *frame_len = m.F;
    if (n_soft) *n_soft = (size_t)m.code.n_soft;
    if ((rc = check_place("mod", m.F, m.tx10, false, n_bursts, start_base, start_step, n_out)) != SFE_OK) return rc;
    if (n_bursts > 0) {
        if (!bytes) {
            set_error("mod: null bytes with bursts to modulate");
            return SFE_EINVAL;
        }
        if (in_stride < m.nbytes()) {
            set_error("mod: in_stride %zu < ceil(n_info / 8) = %zu", in_stride, m.nbytes());
            return SFE_ERANGE;
        }
    }
    if (!out || n_out == 0) return SFE_OK;
    std::vector<v2f> tmp, s;
    v2f *y = static_cast<v2f *>(out);
    if (m.tx10) {
        tmp.resize(n_out);
        y = tmp.data();
    }
    for (size_t i = 0; i < n_out; i++) y[i] = v2f{0.0f, 0.0f};
    for (size_t b = 0; b < n_bursts; b++) {
        mod_symbols_host(m, bytes + b * in_stride, s);
        mod_frame_host(m, s, y + start_base + (int64_t)b * (n_bursts > 1 ? start_step : 0));
    }
    // the wire format's law is ofdmmod_law.h's: the same quantiser, the same groups; omc is v2f's layout
    static_assert(sizeof(omc) == sizeof(v2f) && alignof(omc) == alignof(v2f), "om_tx10_host reads v2f samples");
    if (m.tx10) om_tx10_host(reinterpret_cast<const omc *>(y), n_out, static_cast<uint8_t *>(out));
    return SFE_OK;
}

int sfe_dsp_mod_create(int K, int n_gen, const uint32_t *gen, const uint8_t *keep, int P, int terminated, int n_info, int order,
                       const float *preamble, int n_pre, int sps, const float *taps, int n_taps, float amp, int out_fmt, int device,
                       sfe_mod_t *out)
{
    if (!out) return SFE_EINVAL;
    *out = nullptr;
    std::unique_ptr<Mod> p(new (std::nothrow) Mod);
    if (!p) return SFE_ENOMEM;
    int rc = mod_check(K, n_gen, gen, keep, P, terminated, n_info, order, preamble, n_pre, sps, taps, n_taps, amp, out_fmt, &p->shape);
    if (rc != SFE_OK) return rc;
    CreateScope scope(device);
    if (scope.rc != SFE_OK) return scope.rc;
    p->device = device;
    if ((rc = p->d_taps.upload(p->shape.taps)) != SFE_OK) return rc;
    const v2f none{0.0f, 0.0f};
    if ((rc = n_pre ? p->d_pre.upload(p->shape.pre) : p->d_pre.upload(&none, 1)) != SFE_OK) return rc;
    *out = p.release();
    return SFE_OK;
}

int sfe_dsp_mod_process_stream(sfe_mod_t h, const void *d_bytes, size_t in_stride, size_t n_bursts, int64_t start_base, int64_t start_step,
                               void *d_out, size_t n_out, size_t *n_written, sfe_stream_t stream)
{
    static const char who[] = "mod_process_stream";
    Mod *p = stream_handle(as_mod(h), who, n_written, "n_written");
    if (!p) return SFE_EINVAL;
    const ModShape &m = p->shape;
    static const FrameNouns nouns{"ceil(n_info / 8) = ", "", "payloads'", "cf32 output 8 B; TX10 output and payload bytes need none"};
    bool go;
    int rc = check_frames(who, nouns, m.F, m.tx10, false, d_bytes, in_stride, m.nbytes(), 1, n_bursts, start_base, start_step, d_out, n_out, &go);
    if (rc != SFE_OK || !go) return rc;
    const long long nb = (long long)n_bursts;
    const long long last_end = nb ? start_base + (nb - 1) * (nb > 1 ? start_step : 0) + m.F : 0;
    ModArgs a{};
    a.n_lead = tiles_of(nb ? start_base : (long long)n_out);
    a.tiles_per_slot = nb ? tiles_of(nb > 1 ? start_step : m.F) : 0;
    const __int128 n_tiles = (__int128)a.n_lead + (__int128)nb * a.tiles_per_slot + (nb ? tiles_of((long long)n_out - last_end) : 0);
    if (n_tiles >= ((__int128)1 << 31)) {
        set_error("mod_process_stream: the call's %d-sample tiles must number below 2^31", MOD_TILE);
        return SFE_EINVAL;
    }
    SFE_ON_DEVICE(p->device);
    const VitCode &c = m.code;
    a.bytes = static_cast<const uint8_t *>(d_bytes), a.out = d_out, a.taps = p->d_taps, a.pre = p->d_pre;
    a.in_stride = (long long)in_stride, a.start_base = nb ? start_base : 0, a.start_step = nb > 1 ? start_step : 0;
    a.n_out = (long long)n_out, a.n_bursts = nb;
    for (int j = 0; j < VIT_MAX_GEN; j++) a.gen[j] = c.gen[j];
    a.K = c.K, a.n_gen = c.n, a.P = c.P, a.per_period = c.per_period, a.n_info = c.n_info, a.n_soft = c.n_soft;
    a.order = m.order, a.Lp = m.Lp, a.N = m.N, a.sps = m.sps, a.n_taps = m.n_taps, a.Q = m.Q, a.F = m.F, a.tx10 = m.tx10;
    a.a = m.a;
    std::memcpy(a.pos, m.pos, sizeof a.pos);
    if ((rc = launch_mod(a, (long long)n_tiles, (hipStream_t)stream)) != SFE_OK) return rc;
    *n_written = n_out;
    return SFE_OK;
}

int sfe_dsp_mod_destroy(sfe_mod_t h) { return destroy_handle(as_mod(h)); }

}  // extern "C"
