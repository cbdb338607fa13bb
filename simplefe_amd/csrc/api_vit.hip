// api_vit.hip -- the Viterbi-decoder handle behind sfe_vit_t, sfe_dsp_vit_* (include/sfe_dsp.h).  Host code only; the
// kernel is in vit.hip.  Here: the checks, the encoder, and the host twin of the kernel's law (sfe_dsp_vit_plan: the CPU
// fallback and the reference of the device's bits -- the same float32 additions and comparisons in the same order).
#include <cfloat>
#include <cmath>
#include <cstring>

#include "host.h"
#include "block.h"
#include "vit.h"
#include "vit_code.h"

namespace sfe {

// the code alone: what encode needs, and what the modulator (api_mod.hip) shares; `who` is the message prefix
int vit_check_code(const char *who, int K, int n_gen, const uint32_t *gen, const uint8_t *keep, int P, int terminated, size_t n_info, VitCode *c)
{
    if (K < VIT_MIN_K || K > VIT_MAX_K) {
        set_error("%s: K = %d must be in [%d, %d]", who, K, VIT_MIN_K, VIT_MAX_K);
        return SFE_EINVAL;
    }
    if (n_gen < VIT_MIN_GEN || n_gen > VIT_MAX_GEN) {
        set_error("%s: n_gen = %d must be in [%d, %d]", who, n_gen, VIT_MIN_GEN, VIT_MAX_GEN);
        return SFE_EINVAL;
    }
    if (!gen) {
        set_error("%s: null generators", who);
        return SFE_EINVAL;
    }
    for (int j = 0; j < n_gen; j++)
        if (gen[j] == 0 || gen[j] >= (1u << K)) {
            set_error("%s: generator %d = 0%o must be in (0, 2^K = %u)", who, j, gen[j], 1u << K);
            return SFE_EINVAL;
        }
    if (terminated != 0 && terminated != 1) {
        set_error("%s: terminated = %d must be 0 (truncated) or 1 (K - 1 zero bits follow the payload)", who, terminated);
        return SFE_EINVAL;
    }
    if (n_info < 1 || n_info > (size_t)VIT_MAX_INFO) {
        set_error("%s: n_info = %zu must be in [1, %d]", who, n_info, VIT_MAX_INFO);
        return SFE_EINVAL;
    }
    c->K = K, c->n = n_gen, c->terminated = terminated, c->n_info = (int)n_info;
    for (int j = 0; j < n_gen; j++) c->gen[j] = gen[j];
    c->T = vit_steps(K, terminated, (int)n_info);
    if (!keep) {
        c->P = 1;
        c->keep_lo = (1ull << n_gen) - 1ull;
    } else {
        if (P < 1 || P > VIT_MAX_PERIOD) {
            set_error("%s: puncturing period P = %d must be in [1, %d]", who, P, VIT_MAX_PERIOD);
            return SFE_EINVAL;
        }
        c->P = P;
        for (int tp = 0; tp < P; tp++)
            for (int j = 0; j < n_gen; j++) {
                const uint8_t k = keep[tp * n_gen + j];
                if (k > 1) {
                    set_error("%s: keep[%d][%d] = %d must be 0 or 1", who, tp, j, (int)k);
                    return SFE_EINVAL;
                }
                if (k) (4 * tp + j < 64 ? c->keep_lo : c->keep_hi) |= 1ull << ((4 * tp + j) & 63);
            }
    }
    c->per_period = __builtin_popcountll(c->keep_lo) + __builtin_popcountll(c->keep_hi);
    if (c->per_period == 0) {
        set_error("%s: the puncturing pattern keeps no position", who);
        return SFE_EINVAL;
    }
    long long ns = (long long)(c->T / c->P) * c->per_period;
    for (int tp = 0; tp < c->T % c->P; tp++)
        for (int j = 0; j < n_gen; j++) ns += c->kept(tp, j);
    if (ns == 0) {
        set_error("%s: the puncturing pattern keeps none of the burst's T = %d steps' positions", who, c->T);
        return SFE_EINVAL;
    }
    c->n_soft = (int)ns;
    return SFE_OK;
}

namespace {

constexpr int VIT_MAX_SKIP = 1 << 24;
// vit_process_stream's words for check_rows (call_checks.h); a record is 8 bytes
constexpr RowNouns VIT_NOUNS{"n_bursts", "elements of a burst's row", "ceil(n_info / 8) = ", "", "soft values 4 B, symbols 8 B, records and statuses 4 B", 8};

// what plan and create validate
int vit_check(int K, int n_gen, const uint32_t *gen, const uint8_t *keep, int P, int terminated, int n_info, int in_mode, int skip, VitCode *c)
{
    const int rc = vit_check_code("vit", K, n_gen, gen, keep, P, terminated, n_info < 0 ? 0 : (size_t)n_info, c);
    if (rc != SFE_OK) return rc;
    if (in_mode != SFE_VIT_IN_SOFT && in_mode != SFE_VIT_IN_BPSK && in_mode != SFE_VIT_IN_QPSK) {
        set_error("vit: in_mode = %d must be SFE_VIT_IN_SOFT, SFE_VIT_IN_BPSK or SFE_VIT_IN_QPSK", in_mode);
        return SFE_EINVAL;
    }
    if (skip < 0 || skip > VIT_MAX_SKIP || (in_mode == SFE_VIT_IN_SOFT && skip != 0)) {
        set_error("vit: skip = %d must be in [0, %d], and 0 with SFE_VIT_IN_SOFT", skip, VIT_MAX_SKIP);
        return SFE_EINVAL;
    }
    c->in_mode = in_mode, c->skip = skip;
    if (!vit_fits(K, c->T, n_info)) {
        set_error("vit: the survivors of one burst, T * max(2^(K-1), 64) / 8 = %zu bytes, and its packed bits, %zu bytes, exceed the %zu bytes of LDS a launch may "
                  "ask for (K = %d, T = %d)", vit_surv_bytes(K, c->T), vit_bits_bytes(n_info), VIT_LDS_BUDGET, K, c->T);
        return SFE_EINVAL;
    }
    return SFE_OK;
}

void vit_fail_host(const VitCode &c, int st, uint8_t *bytes, uint32_t *rec, int *status)
{
    std::memset(bytes, 0, ((size_t)c.n_info + 7) / 8);
    if (rec) rec[0] = VIT_QNAN, rec[1] = 0u;
    if (status) *status = st;
}

// Scratch of the host decoder, made once per plan call.
struct VitWork {
    std::vector<float> pm, nw, r;
    std::vector<uint8_t> lab0, lab1, surv, word;
};

// The law of include/sfe_dsp.h on one burst: float32 additions and comparisons, one IEEE operation each.  row: the
// burst's row from soft value 0 on, soft value i at row[i mul].
void vit_solve_host(const VitCode &c, VitWork &w, const float *row, int mul, uint8_t *bytes, uint32_t *rec, int *status)
{
    const int S = c.S(), T = c.T, n = c.n;
    for (int i = 0; i < c.n_soft; i++)
        if (!std::isfinite(row[(size_t)i * mul])) return vit_fail_host(c, VIT_NOT_FINITE, bytes, rec, status);
    // the soft values with the punctured positions filled in with +0
    w.r.assign((size_t)T * n, 0.0f);
    for (int t = 0, i = 0; t < T; t++)
        for (int j = 0; j < n; j++)
            if (c.kept(t % c.P, j)) w.r[(size_t)t * n + j] = row[(size_t)(i++) * mul];
    w.pm.assign(S, -INFINITY);
    w.nw.assign(S, 0.0f);
    w.pm[0] = 0.0f;
    w.surv.assign((size_t)T * S, 0);
    float bm[1 << VIT_MAX_GEN];
    for (int t = 0; t < T; t++) {
        const float *r = &w.r[(size_t)t * n];
        for (unsigned l = 0; l < (1u << n); l++) {         // ((+-r_0) + (+-r_1)) + ..., minus where the label's bit is 1
            float acc = (l & 1u) ? -r[0] : r[0];
            for (int j = 1; j < n; j++) acc = acc + ((l >> j) & 1u ? -r[j] : r[j]);
            bm[l] = acc;
        }
        uint8_t *d = &w.surv[(size_t)t * S];
        for (int s = 0; s < S; s++) {
            const int p0 = s >> 1, p1 = p0 | (S >> 1);
            const float c0 = w.pm[p0] + bm[w.lab0[s]], c1 = w.pm[p1] + bm[w.lab1[s]];
            d[s] = c1 > c0;
            w.nw[s] = d[s] ? c1 : c0;
        }
        w.pm.swap(w.nw);
    }
    int end = 0;
    if (!c.terminated)
        for (int s = 1; s < S; s++)
            if (w.pm[s] > w.pm[end]) end = s;
    w.word.assign(T, 0);
    for (int t = T - 1, s = end; t >= 0; t--) {
        w.word[t] = s & 1;
        s = (s >> 1) | ((int)w.surv[(size_t)t * S + s] << (c.K - 2));
    }
    std::memset(bytes, 0, ((size_t)c.n_info + 7) / 8);
    for (int t = 0; t < c.n_info; t++) bytes[t >> 3] |= (uint8_t)(w.word[t] << (7 - (t & 7)));
    if (rec) {
        uint32_t cnt = 0;
        unsigned reg = 0;
        for (int t = 0; t < T; t++) {
            reg = ((reg << 1) | (t < c.n_info ? w.word[t] : 0)) & ((1u << c.K) - 1u);
            const unsigned l = c.label(reg);
            for (int j = 0; j < n; j++) {
                const float v = w.r[(size_t)t * n + j];
                cnt += ((l >> j) & 1u) ? (v > 0.0f) : (v < 0.0f);
            }
        }
        std::memcpy(&rec[0], &w.pm[end], 4);
        rec[1] = cnt;
    }
    if (status) *status = VIT_OK;
}

struct Vit {
    static constexpr uint32_t MAGIC = 0x56495431u;   // 'VIT1'
    uint32_t magic = MAGIC;
    int device = 0;
    VitCode code;       // never changes after create: a call pins nothing a later call could move
    int staged = 0, waves = 1;
};

Vit *as_vit(void *h) { return as_handle<Vit>(h, "Viterbi-decoder"); }

VitArgs vit_args(const Vit &v)
{
    const VitCode &c = v.code;
    VitArgs a{};
    for (int j = 0; j < VIT_MAX_GEN; j++) a.gen[j] = c.gen[j];
    a.keep_lo = c.keep_lo, a.keep_hi = c.keep_hi;
    a.K = c.K, a.n_gen = c.n, a.P = c.P, a.per_period = c.per_period, a.terminated = c.terminated, a.n_info = c.n_info, a.T = c.T, a.n_soft = c.n_soft;
    a.in_off = c.in_off(), a.in_mul = c.in_mul();
    a.staged = v.staged, a.waves = v.waves;
    return a;
}

}  // namespace
}  // namespace sfe

using namespace sfe;

extern "C" {

int sfe_dsp_vit_encode(int K, int n_gen, const uint32_t *gen, const uint8_t *keep, int P, int terminated, const uint8_t *bits,
                       size_t n_info, uint8_t *coded, size_t *n_coded)
{
    if (n_coded) *n_coded = 0;
    VitCode c;
    const int rc = vit_check_code("vit", K, n_gen, gen, keep, P, terminated, n_info, &c);
    if (rc != SFE_OK) return rc;
    if (!n_coded) {
        set_error("vit: null n_coded");
        return SFE_EINVAL;
    }
    *n_coded = (size_t)c.n_soft;
    if (!coded) return SFE_OK;
    if (!bits) {
        set_error("vit: null bits with coded bits to write");
        return SFE_EINVAL;
    }
    for (size_t t = 0; t < n_info; t++)
        if (bits[t] > 1) {
            set_error("vit: bit %zu = %d must be 0 or 1", t, (int)bits[t]);
            return SFE_EINVAL;
        }
    unsigned reg = 0;
    size_t i = 0;
    for (int t = 0; t < c.T; t++) {
        reg = ((reg << 1) | (t < c.n_info ? bits[t] : 0u)) & ((1u << K) - 1u);
        const unsigned l = c.label(reg);
        for (int j = 0; j < n_gen; j++)
            if (c.kept(t % c.P, j)) coded[i++] = (uint8_t)((l >> j) & 1u);
    }
    return SFE_OK;
}

int sfe_dsp_vit_footprint(int K, int n_gen, int terminated, int n_info, size_t *lds_bytes, int *staged, int *bursts_per_group)
{
    const uint32_t one[VIT_MAX_GEN] = {1, 1, 1, 1};
    VitCode c;
    const int rc = vit_check_code("vit", K, n_gen, one, nullptr, 1, terminated, n_info < 0 ? 0 : (size_t)n_info, &c);
    if (rc != SFE_OK) return rc;
    if (lds_bytes) *lds_bytes = vit_base_bytes(K, c.T, n_info);
    if (staged) *staged = vit_staged(K, n_gen, c.T, n_info) ? 1 : 0;
    if (bursts_per_group) *bursts_per_group = vit_fits(K, c.T, n_info) ? vit_waves(K, n_gen, c.T, n_info) : 0;
    return SFE_OK;
}

int sfe_dsp_vit_plan(int K, int n_gen, const uint32_t *gen, const uint8_t *keep, int P, int terminated, int n_info, int in_mode,
                     int skip, const float *in, size_t in_stride, const int *status_in, size_t n_bursts, uint8_t *bytes,
                     size_t out_stride, uint32_t *record, int *status, size_t *n_soft)
{
    if (n_soft) *n_soft = 0;
    VitCode c;
    const int rc = vit_check(K, n_gen, gen, keep, P, terminated, n_info, in_mode, skip, &c);
    if (rc != SFE_OK) return rc;
    if (n_soft) *n_soft = (size_t)c.n_soft;
    if (!in || n_bursts == 0) return SFE_OK;
    if (!bytes) {
        set_error("vit: null bytes with soft values to decode");
        return SFE_EINVAL;
    }
    if (n_bursts >= ((size_t)1 << 31)) {
        set_error("vit: n_bursts = %zu must be below 2^31", n_bursts);
        return SFE_EINVAL;
    }
    const size_t nbytes = ((size_t)n_info + 7) / 8;
    if (in_stride < c.row_elems() || out_stride < nbytes) {
        set_error("vit: in_stride %zu < the %zu elements of a burst's row, or out_stride %zu < ceil(n_info / 8) = %zu", in_stride, c.row_elems(),
                  out_stride, nbytes);
        return SFE_ERANGE;
    }
    VitWork w;
    const int S = c.S();
    w.lab0.resize(S), w.lab1.resize(S);
    for (int s = 0; s < S; s++) w.lab0[s] = (uint8_t)c.label((unsigned)s), w.lab1[s] = (uint8_t)c.label((unsigned)(s | S));
    for (size_t b = 0; b < n_bursts; b++) {
        uint8_t *by = bytes + b * out_stride;
        uint32_t *rec = record ? record + 2 * b : nullptr;
        int *st = status ? status + b : nullptr;
        if (status_in && status_in[b] != 0) vit_fail_host(c, VIT_UPSTREAM, by, rec, st);
        else vit_solve_host(c, w, in + b * in_stride * c.elem_floats() + c.in_off(), c.in_mul(), by, rec, st);
    }
    return SFE_OK;
}

int sfe_dsp_vit_create(int K, int n_gen, const uint32_t *gen, const uint8_t *keep, int P, int terminated, int n_info, int in_mode,
                       int skip, int device, sfe_vit_t *out)
{
    if (!out) return SFE_EINVAL;
    *out = nullptr;
    VitCode c;
    int rc = vit_check(K, n_gen, gen, keep, P, terminated, n_info, in_mode, skip, &c);
    if (rc != SFE_OK) return rc;
    CreateScope scope(device);
    if (scope.rc != SFE_OK) return scope.rc;
    std::unique_ptr<Vit> p(new (std::nothrow) Vit);
    if (!p) return SFE_ENOMEM;
    p->device = device;
    p->code = c;
    p->staged = vit_staged(K, n_gen, c.T, n_info) ? 1 : 0;
    p->waves = vit_waves(K, n_gen, c.T, n_info);
    if ((rc = launch_vit(vit_args(*p), nullptr, true)) != SFE_OK) return rc;
    *out = p.release();
    return SFE_OK;
}

int sfe_dsp_vit_process_stream(sfe_vit_t h, const void *d_in, size_t in_stride, const void *d_status_in, size_t n_bursts, void *d_bits,
                               size_t out_stride, void *d_rec, void *d_status, size_t *n_out, sfe_stream_t stream)
{
    static const char who[] = "vit_process_stream";
    Vit *p = stream_handle(as_vit(h), who, n_out);
    if (!p) return SFE_EINVAL;
    const VitCode &c = p->code;
    bool go;
    int rc = check_rows(who, VIT_NOUNS, n_bursts, d_in, in_stride, c.row_elems(), 4 * (size_t)c.elem_floats(), d_status_in, d_bits, out_stride,
                        ((size_t)c.n_info + 7) / 8, d_rec, d_status, &go);
    if (rc != SFE_OK || !go) return rc;
    SFE_ON_DEVICE(p->device);
    VitArgs a = vit_args(*p);
    a.in = static_cast<const float *>(d_in);
    a.status_in = static_cast<const int *>(d_status_in);
    a.bits = static_cast<uint8_t *>(d_bits);
    a.rec = static_cast<uint32_t *>(d_rec);
    a.status = static_cast<int *>(d_status);
    a.in_stride = (long long)in_stride * c.elem_floats();
    a.out_stride = (long long)out_stride;
    a.n_bursts = (long long)n_bursts;
    rc = launch_vit(a, (hipStream_t)stream);
    if (rc != SFE_OK) return rc;
    *n_out = n_bursts;
    return SFE_OK;
}

int sfe_dsp_vit_destroy(sfe_vit_t h) { return destroy_handle(as_vit(h)); }

}  // extern "C"
