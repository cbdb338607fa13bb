// api_crc.hip -- the frame check's handle behind sfe_crc_t, sfe_dsp_crc_* (include/sfe_dsp.h), the host plan and the host's
// sequence generator.  Host code only; the kernels are crc.hip, the law both run is crc_law.h.
#include <cstring>

#include "host.h"
#include "block.h"
#include "crc.h"
#include "crc_law.h"

namespace sfe {
namespace {

struct Crc {
    static constexpr uint32_t MAGIC = 0x43524331u;   // 'CRC1'
    uint32_t magic = MAGIC;
    int device = 0;
    CrcLaw law;                 // never changes after create
    uint32_t init_term = 0;
    DevBuf<uint8_t> d_pn;       // the sequence in frame coordinates, zeros up to a multiple of 4 behind it; empty without a scrambler
    DevBuf<uint32_t> d_tab;     // the two classes' columns and weights (crc.h)
};

Crc *as_crc(void *h) { return as_handle<Crc>(h, "frame-check"); }

// what plan and create validate
int crc_checked(int width, uint32_t poly, uint32_t init, int reflect, uint32_t xorout, int pn_m, uint32_t pn_taps, uint32_t pn_seed, int payload,
                CrcLaw *c)
{
    char msg[200];
    if (crc_check_args(width, poly, init, reflect, xorout, pn_m, pn_taps, pn_seed, payload, c, msg, sizeof msg) != 0) {
        set_error("crc: %s", msg);
        return SFE_EINVAL;
    }
    return SFE_OK;
}

CrcArgs crc_args(const Crc &p, int check)
{
    CrcArgs a{};
    a.pn = p.d_pn;
    a.tab = p.d_tab;
    a.law = p.law;
    a.init_term = p.init_term;
    a.check = check;
    return a;
}

// the stream calls' words for check_rows (call_checks.h); a record is 8 bytes
constexpr RowNouns CRC_NOUNS{"n_frames", "bytes read per frame", "the ", " bytes written per frame",
                             "records and statuses 4 B; payloads and frames need none", 8};

}  // namespace
}  // namespace sfe

using namespace sfe;

extern "C" {

int sfe_dsp_crc_pn_bytes(int m, uint32_t taps, uint32_t seed, size_t n, uint8_t *out)
{
    if (m == 0) {
        set_error("crc: pn_m = 0 names no sequence");
        return SFE_EINVAL;
    }
    CrcLaw c;
    const int rc = crc_checked(0, 0, 0, 0, 0, m, taps, seed, 1, &c);
    if (rc != SFE_OK) return rc;
    if (n && !out) {
        set_error("crc: pn_bytes: null buffer");
        return SFE_EINVAL;
    }
    crc_pn_bytes(m, taps, seed, n, out);
    return SFE_OK;
}

int sfe_dsp_crc_plan(int width, uint32_t poly, uint32_t init, int reflect, uint32_t xorout, int pn_m, uint32_t pn_taps, uint32_t pn_seed,
                     int payload_bytes, int check, const uint8_t *in, size_t in_stride, const int *status_in, size_t n_frames, uint8_t *out,
                     size_t out_stride, uint32_t *record, int *status, int *frame_bytes)
{
    if (frame_bytes) *frame_bytes = 0;
    CrcLaw c;
    const int rc = crc_checked(width, poly, init, reflect, xorout, pn_m, pn_taps, pn_seed, payload_bytes, &c);
    if (rc != SFE_OK) return rc;
    if (check != 0 && check != 1) {
        set_error("crc: check = %d is neither 0 nor 1", check);
        return SFE_EINVAL;
    }
    const size_t P = (size_t)c.payload, Fb = (size_t)c.frame_bytes();
    if (frame_bytes) *frame_bytes = (int)Fb;
    if (!in || n_frames == 0) return SFE_OK;
    if (n_frames >= ((size_t)1 << 31)) {
        set_error("crc: n_frames = %zu must be below 2^31", n_frames);
        return SFE_EINVAL;
    }
    const size_t in_row = check ? Fb : P, out_row = check ? P : Fb;
    if (in_stride < in_row || (out && out_stride < out_row)) {
        set_error("crc: in_stride %zu < the %zu bytes read per frame, or out_stride %zu < the %zu bytes written per frame", in_stride, in_row,
                  out_stride, out_row);
        return SFE_ERANGE;
    }
    CrcTable T;
    crc_table(c, &T);
    std::vector<uint8_t> pn;
    if (c.pn_m) {
        pn.resize(Fb);
        crc_pn_bytes(c.pn_m, c.pn_taps, c.pn_seed, Fb, pn.data());
    }
    const uint8_t *seq = c.pn_m ? pn.data() : nullptr;
    for (size_t b = 0; b < n_frames; b++) {
        if (check)
            crc_check_frame(c, T, seq, in + b * in_stride, status_in && status_in[b] != 0, out ? out + b * out_stride : nullptr,
                            record ? record + 2 * b : nullptr, status ? status + b : nullptr);
        else
            crc_append_frame(c, T, seq, in + b * in_stride, out ? out + b * out_stride : nullptr);
    }
    return SFE_OK;
}

int sfe_dsp_crc_create(int width, uint32_t poly, uint32_t init, int reflect, uint32_t xorout, int pn_m, uint32_t pn_taps, uint32_t pn_seed,
                       int payload_bytes, int device, sfe_crc_t *out)
{
    if (!out) return SFE_EINVAL;
    *out = nullptr;
    std::unique_ptr<Crc> p(new (std::nothrow) Crc);
    if (!p) return SFE_ENOMEM;
    int rc = crc_checked(width, poly, init, reflect, xorout, pn_m, pn_taps, pn_seed, payload_bytes, &p->law);
    if (rc != SFE_OK) return rc;
    CreateScope scope(device);
    if (scope.rc != SFE_OK) return scope.rc;
    p->device = device;
    const CrcLaw &c = p->law;
    const uint32_t polyL = c.polyL();
    p->init_term = crc_mulmod(c.initL(), crc_xpow(8ull * (uint64_t)c.payload, polyL), polyL);
    std::vector<uint32_t> tab(CRC_TAB_WORDS, 0u);
    crc_class_constants(polyL, CRC_SHORT_T, &tab[CRC_TAB_SHORT]);
    crc_class_constants(polyL, CRC_LONG_T, &tab[CRC_TAB_LONG]);
    if ((rc = p->d_tab.upload(tab)) != SFE_OK) return rc;
    if (c.pn_m) {
        const size_t Fb = (size_t)c.frame_bytes();
        std::vector<uint8_t> pn((Fb + 3) / 4 * 4, 0);
        crc_pn_bytes(c.pn_m, c.pn_taps, c.pn_seed, Fb, pn.data());
        if ((rc = p->d_pn.upload(pn)) != SFE_OK) return rc;
    }
    *out = p.release();
    return SFE_OK;
}

int sfe_dsp_crc_append_stream(sfe_crc_t h, const void *d_payload, size_t in_stride, size_t n_frames, void *d_frame, size_t out_stride,
                              size_t *n_out, sfe_stream_t stream)
{
    static const char who[] = "crc_append_stream";
    Crc *p = stream_handle(as_crc(h), who, n_out);
    if (!p) return SFE_EINVAL;
    bool go;
    int rc = check_rows(who, CRC_NOUNS, n_frames, d_payload, in_stride, (size_t)p->law.payload, 1, nullptr, d_frame, out_stride,
                        (size_t)p->law.frame_bytes(), nullptr, nullptr, &go);
    if (rc != SFE_OK || !go) return rc;
    SFE_ON_DEVICE(p->device);
    CrcArgs a = crc_args(*p, 0);
    a.in = static_cast<const uint8_t *>(d_payload);
    a.out = static_cast<uint8_t *>(d_frame);
    a.in_stride = (long long)in_stride, a.out_stride = (long long)out_stride, a.n_frames = (long long)n_frames;
    if ((rc = launch_crc(a, (hipStream_t)stream)) != SFE_OK) return rc;
    *n_out = n_frames;
    return SFE_OK;
}

int sfe_dsp_crc_check_stream(sfe_crc_t h, const void *d_frame, size_t in_stride, const void *d_status_in, size_t n_frames, void *d_out,
                             size_t out_stride, void *d_rec, void *d_status, size_t *n_out, sfe_stream_t stream)
{
    static const char who[] = "crc_check_stream";
    Crc *p = stream_handle(as_crc(h), who, n_out);
    if (!p) return SFE_EINVAL;
    if (!d_out && !d_rec && !d_status) {
        set_error("%s: d_out, d_rec and d_status are all null: a call with no output", who);
        return SFE_EINVAL;
    }
    bool go;
    int rc = check_rows(who, CRC_NOUNS, n_frames, d_frame, in_stride, (size_t)p->law.frame_bytes(), 1, d_status_in, d_out, out_stride,
                        (size_t)p->law.payload, d_rec, d_status, &go, true);
    if (rc != SFE_OK || !go) return rc;
    SFE_ON_DEVICE(p->device);
    CrcArgs a = crc_args(*p, 1);
    a.in = static_cast<const uint8_t *>(d_frame);
    a.status_in = static_cast<const int *>(d_status_in);
    a.out = static_cast<uint8_t *>(d_out);
    a.rec = static_cast<uint32_t *>(d_rec);
    a.status = static_cast<int *>(d_status);
    a.in_stride = (long long)in_stride, a.out_stride = (long long)out_stride, a.n_frames = (long long)n_frames;
    if ((rc = launch_crc(a, (hipStream_t)stream)) != SFE_OK) return rc;
    *n_out = n_frames;
    return SFE_OK;
}

int sfe_dsp_crc_destroy(sfe_crc_t h) { return destroy_handle(as_crc(h)); }

}  // extern "C"
