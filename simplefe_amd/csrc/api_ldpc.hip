// api_ldpc.hip -- the quasi-cyclic LDPC code's handle behind sfe_ldpc_t, sfe_dsp_ldpc_* (include/sfe_dsp.h), and the host
// plan.  Host code only; the kernels are ldpc.hip, the law both run is ldpc_law.h.
#include <cstring>
#include <mutex>

#include "host.h"
#include "block.h"
#include "ldpc.h"
#include "ldpc_law.h"

namespace sfe {
namespace {

constexpr int LDPC_MAX_SKIP = 1 << 24;

// what plan and create validate beside the matrix
struct LdpcParams {
    float scale = 0.0f;
    int a = 0, beta = 0, max_iter = 0, in_mode = 0, skip = 0;
    int elem_floats() const { return in_mode == SFE_VIT_IN_SOFT ? 1 : 2; }
    int in_off() const { return in_mode == SFE_VIT_IN_SOFT ? 0 : 2 * skip; }
    int in_mul() const { return in_mode == SFE_VIT_IN_BPSK ? 2 : 1; }
    size_t row_elems(int n) const       // elements of the mode's type a codeword's row must hold
    {
        if (in_mode == SFE_VIT_IN_SOFT) return (size_t)n;
        return (size_t)skip + (in_mode == SFE_VIT_IN_BPSK ? (size_t)n : ((size_t)n + 1) / 2);
    }
};

// A validated code with its encoder's table.  The elimination behind `encodable` takes a noticeable fraction of a second
// at n = 8192, and the plan is a stateless call: the latest codes are kept, keyed by their whole base matrix.
std::shared_ptr<const LdpcCode> ldpc_code(int mb, int nb, int Z, const int16_t *shift, int *rc)
{
    struct Entry {
        int Z;
        std::vector<int16_t> shift;
        std::shared_ptr<const LdpcCode> code;
    };
    static std::mutex mu;
    static std::vector<Entry> kept;
    auto c = std::make_shared<LdpcCode>();
    char msg[160];
    if (ldpc_check(mb, nb, Z, shift, c.get(), msg, sizeof msg) != 0) {
        set_error("ldpc: %s", msg);
        *rc = SFE_EINVAL;
        return nullptr;
    }
    *rc = SFE_OK;
    const std::vector<int16_t> key(shift, shift + (size_t)mb * nb);
    {
        std::lock_guard<std::mutex> lock(mu);
        for (const Entry &e : kept)
            if (e.Z == Z && e.code->mb == mb && e.code->nb == nb && e.shift == key) return e.code;
    }
    ldpc_build_encoder(c.get());
    std::lock_guard<std::mutex> lock(mu);
    if (kept.size() >= 16) kept.erase(kept.begin());
    kept.push_back(Entry{Z, key, c});
    return c;
}

int ldpc_params(float scale, int a, int beta, int max_iter, int in_mode, int skip, LdpcParams *p)
{
    char msg[160];
    if (ldpc_check_params(scale, a, beta, max_iter, msg, sizeof msg) != 0) {
        set_error("ldpc: %s", msg);
        return SFE_EINVAL;
    }
    if (in_mode != SFE_VIT_IN_SOFT && in_mode != SFE_VIT_IN_BPSK && in_mode != SFE_VIT_IN_QPSK) {
        set_error("ldpc: in_mode = %d must be SFE_VIT_IN_SOFT, SFE_VIT_IN_BPSK or SFE_VIT_IN_QPSK", in_mode);
        return SFE_EINVAL;
    }
    if (skip < 0 || skip > LDPC_MAX_SKIP || (in_mode == SFE_VIT_IN_SOFT && skip != 0)) {
        set_error("ldpc: skip = %d must be in [0, %d], and 0 with SFE_VIT_IN_SOFT", skip, LDPC_MAX_SKIP);
        return SFE_EINVAL;
    }
    p->scale = scale, p->a = a, p->beta = beta, p->max_iter = max_iter, p->in_mode = in_mode, p->skip = skip;
    return SFE_OK;
}

struct Ldpc {
    static constexpr uint32_t MAGIC = 0x4c445031u;   // 'LDP1'
    uint32_t magic = MAGIC;
    int device = 0;
    std::shared_ptr<const LdpcCode> code;       // never changes after create
    LdpcParams par;
    LdpcLayout lay{};
    int tab_cells = 0, tab_inv = 0;
    DevBuf<uint32_t> d_tab;                     // row starts, cells, the inverse's blocks (ldpc.h)
};

Ldpc *as_ldpc(void *h) { return as_handle<Ldpc>(h, "LDPC"); }

LdpcArgs ldpc_args(const Ldpc &p)
{
    const LdpcCode &c = *p.code;
    LdpcArgs a{};
    a.tab = p.d_tab;
    a.mb = c.mb, a.Z = c.Z, a.n = c.n, a.k = c.k, a.n_cells = (int)c.cells.size(), a.tab_cells = p.tab_cells, a.tab_inv = p.tab_inv, a.Zw = c.Zw;
    a.in_off = p.par.in_off(), a.in_mul = p.par.in_mul();
    a.scale = p.par.scale, a.a = p.par.a, a.beta = p.par.beta, a.max_iter = p.par.max_iter;
    a.lay = p.lay;
    return a;
}

// the stream calls' words for check_rows (call_checks.h); a record is 12 bytes
constexpr RowNouns LDPC_NOUNS{"n_words", "elements read per codeword", "the ", " bytes written per codeword",
                              "soft values 4 B, symbols 8 B, records and statuses 4 B; payloads and codewords need none", 12};

}  // namespace
}  // namespace sfe

using namespace sfe;

extern "C" {

int sfe_dsp_ldpc_footprint(int mb, int nb, int Z, const int16_t *shift, size_t *lds_bytes, int *words_per_group)
{
    if (lds_bytes) *lds_bytes = 0;
    if (words_per_group) *words_per_group = 0;
    LdpcCode c;
    char msg[160];
    if (ldpc_check(mb, nb, Z, shift, &c, msg, sizeof msg) != 0) {
        set_error("ldpc: %s", msg);
        return SFE_EINVAL;
    }
    const LdpcLayout l = ldpc_layout(c.n, (int)c.cells.size(), c.mb, c.Z);
    if (lds_bytes) *lds_bytes = l.lds;
    if (words_per_group) *words_per_group = l.group;
    return SFE_OK;
}

int sfe_dsp_ldpc_plan(int mb, int nb, int Z, const int16_t *shift, float scale, int a, int beta, int max_iter, int in_mode, int skip, int encode,
                      const void *in, size_t in_stride, const int *status_in, size_t n_words, uint8_t *out, size_t out_stride, uint32_t *record,
                      int *status, int *n, int *k, int *encodable)
{
    if (n) *n = 0;
    if (k) *k = 0;
    if (encodable) *encodable = 0;
    int rc;
    const std::shared_ptr<const LdpcCode> code = ldpc_code(mb, nb, Z, shift, &rc);
    if (!code) return rc;
    LdpcParams par;
    if ((rc = ldpc_params(scale, a, beta, max_iter, in_mode, skip, &par)) != SFE_OK) return rc;
    if (encode != 0 && encode != 1) {
        set_error("ldpc: encode = %d is neither 0 nor 1", encode);
        return SFE_EINVAL;
    }
    const LdpcCode &c = *code;
    if (n) *n = c.n;
    if (k) *k = c.k;
    if (encodable) *encodable = c.encodable;
    if (!in || n_words == 0) return SFE_OK;
    if (n_words >= ((size_t)1 << 31)) {
        set_error("ldpc: n_words = %zu must be below 2^31", n_words);
        return SFE_EINVAL;
    }
    const size_t in_row = encode ? (size_t)c.k_bytes() : par.row_elems(c.n), out_row = encode ? (size_t)c.n_bytes() : (size_t)c.k_bytes();
    if (in_stride < in_row || (out && out_stride < out_row)) {
        set_error("ldpc: in_stride %zu < the %zu elements read per codeword, or out_stride %zu < the %zu bytes written per codeword", in_stride, in_row,
                  out_stride, out_row);
        return SFE_ERANGE;
    }
    if (encode) {
        if (!c.encodable) {
            set_error("ldpc: the parity part of H (its last m columns) is singular: the code is not encodable");
            return SFE_ESTATE;
        }
        if (out)
            for (size_t b = 0; b < n_words; b++) ldpc_encode_word(c, static_cast<const uint8_t *>(in) + b * in_stride, out + b * out_stride);
        return SFE_OK;
    }
    LdpcWork w;
    const float *x = static_cast<const float *>(in);
    for (size_t b = 0; b < n_words; b++) {
        uint8_t *by = out ? out + b * out_stride : nullptr;
        uint32_t *rec = record ? record + 3 * b : nullptr;
        int *st = status ? status + b : nullptr;
        if (status_in && status_in[b] != 0) ldpc_fail_word(c, LDPC_UPSTREAM, by, rec, st);
        else ldpc_decode_word(c, w, x + b * in_stride * par.elem_floats() + par.in_off(), par.in_mul(), par.scale, par.a, par.beta, par.max_iter, by, rec, st);
    }
    return SFE_OK;
}

int sfe_dsp_ldpc_create(int mb, int nb, int Z, const int16_t *shift, float scale, int a, int beta, int max_iter, int in_mode, int skip, int device,
                        sfe_ldpc_t *out)
{
    if (!out) return SFE_EINVAL;
    *out = nullptr;
    std::unique_ptr<Ldpc> p(new (std::nothrow) Ldpc);
    if (!p) return SFE_ENOMEM;
    int rc;
    p->code = ldpc_code(mb, nb, Z, shift, &rc);
    if (!p->code) return rc;
    if ((rc = ldpc_params(scale, a, beta, max_iter, in_mode, skip, &p->par)) != SFE_OK) return rc;
    CreateScope scope(device);
    if (scope.rc != SFE_OK) return scope.rc;
    p->device = device;
    const LdpcCode &c = *p->code;
    p->lay = ldpc_layout(c.n, (int)c.cells.size(), c.mb, c.Z);
    std::vector<uint32_t> tab;
    for (int r = 0; r <= c.mb; r++) tab.push_back(c.row_start[r]);
    p->tab_cells = (int)tab.size();
    for (const LdpcCell &ce : c.cells) tab.push_back((uint32_t)ce.col | (uint32_t)ce.shift << 16);
    p->tab_inv = (int)tab.size();
    tab.insert(tab.end(), c.inv.begin(), c.inv.end());
    if ((rc = p->d_tab.upload(tab)) != SFE_OK) return rc;
    if ((rc = launch_ldpc_decode(ldpc_args(*p), nullptr, true)) != SFE_OK) return rc;
    *out = p.release();
    return SFE_OK;
}

int sfe_dsp_ldpc_encode_stream(sfe_ldpc_t h, const void *d_payload, size_t in_stride, size_t n_words, void *d_code, size_t out_stride, size_t *n_out,
                               sfe_stream_t stream)
{
    static const char who[] = "ldpc_encode_stream";
    Ldpc *p = stream_handle(as_ldpc(h), who, n_out);
    if (!p) return SFE_EINVAL;
    if (!p->code->encodable) {
        set_error("ldpc_encode_stream: the parity part of H (its last m columns) is singular: the handle's code is not encodable");
        return SFE_ESTATE;
    }
    bool go;
    int rc = check_rows(who, LDPC_NOUNS, n_words, d_payload, in_stride, (size_t)p->code->k_bytes(), 1, nullptr, d_code, out_stride,
                        (size_t)p->code->n_bytes(), nullptr, nullptr, &go);
    if (rc != SFE_OK || !go) return rc;
    SFE_ON_DEVICE(p->device);
    LdpcArgs a = ldpc_args(*p);
    a.payload = static_cast<const uint8_t *>(d_payload);
    a.out = static_cast<uint8_t *>(d_code);
    a.in_stride = (long long)in_stride, a.out_stride = (long long)out_stride, a.n_words = (long long)n_words;
    if ((rc = launch_ldpc_encode(a, (hipStream_t)stream)) != SFE_OK) return rc;
    *n_out = n_words;
    return SFE_OK;
}

int sfe_dsp_ldpc_process_stream(sfe_ldpc_t h, const void *d_in, size_t in_stride, const void *d_status_in, size_t n_words, void *d_bits,
                                size_t out_stride, void *d_rec, void *d_status, size_t *n_out, sfe_stream_t stream)
{
    static const char who[] = "ldpc_process_stream";
    Ldpc *p = stream_handle(as_ldpc(h), who, n_out);
    if (!p) return SFE_EINVAL;
    const LdpcParams &par = p->par;
    bool go;
    int rc = check_rows(who, LDPC_NOUNS, n_words, d_in, in_stride, par.row_elems(p->code->n), 4 * (size_t)par.elem_floats(), d_status_in, d_bits,
                        out_stride, (size_t)p->code->k_bytes(), d_rec, d_status, &go);
    if (rc != SFE_OK || !go) return rc;
    SFE_ON_DEVICE(p->device);
    LdpcArgs a = ldpc_args(*p);
    a.in = static_cast<const float *>(d_in);
    a.status_in = static_cast<const int *>(d_status_in);
    a.out = static_cast<uint8_t *>(d_bits);
    a.rec = static_cast<uint32_t *>(d_rec);
    a.status = static_cast<int *>(d_status);
    a.in_stride = (long long)in_stride * par.elem_floats(), a.out_stride = (long long)out_stride, a.n_words = (long long)n_words;
    if ((rc = launch_ldpc_decode(a, (hipStream_t)stream)) != SFE_OK) return rc;
    *n_out = n_words;
    return SFE_OK;
}

int sfe_dsp_ldpc_destroy(sfe_ldpc_t h) { return destroy_handle(as_ldpc(h)); }

}  // extern "C"
