// api_reed.hip -- the Reed-Solomon outer code's handle behind sfe_reed_t, sfe_dsp_reed_* (include/sfe_dsp.h), and the host
// plan.  Host code only; the kernels are reed.hip, the law both run is reed_law.h.
#include <cstring>

#include "host.h"
#include "block.h"
#include "reed.h"
#include "reed_law.h"

namespace sfe {
namespace {

struct Reed {
    static constexpr uint32_t MAGIC = 0x52454431u;   // 'RED1'
    uint32_t magic = MAGIC;
    int device = 0;
    ReedCode code;              // never changes after create
    int whiten = 0;
    DevBuf<uint8_t> d_tab;      // roots, generator, locators, whitening (reed.h)
};

Reed *as_reed(void *h) { return as_handle<Reed>(h, "Reed-Solomon"); }

// what plan and create validate
int reed_checked(int prim, int fcr, int step, int n, int n_par, int depth, ReedCode *c)
{
    char msg[160];
    if (reed_check(prim, fcr, step, n, n_par, depth, c, msg, sizeof msg) != 0) {
        set_error("reed: %s", msg);
        return SFE_EINVAL;
    }
    return SFE_OK;
}

ReedArgs reed_args(const Reed &r)
{
    const ReedCode &c = r.code;
    ReedArgs a{};
    a.tab = r.d_tab;
    a.prim = c.prim, a.n = c.n, a.n_par = c.n_par, a.k = c.k, a.t = c.t, a.depth = c.depth;
    a.fpb = c.depth >= REED_WAVES ? 1 : REED_WAVES / c.depth;
    a.recip = (65536u + (unsigned)c.depth - 1u) / (unsigned)c.depth;
    a.whiten = r.whiten;
    return a;
}

// the stream calls' words for check_rows (call_checks.h); a record is 8 bytes
constexpr RowNouns REED_NOUNS{"n_frames", "bytes read per frame", "the ", " bytes written per frame",
                              "records and statuses 4 B; payloads and frames need none", 8};

}  // namespace
}  // namespace sfe

using namespace sfe;

extern "C" {

int sfe_dsp_reed_plan(int prim, int fcr, int step, int n, int n_par, int depth, const uint8_t *whiten, int encode, const uint8_t *in,
                      size_t in_stride, const int *status_in, size_t n_frames, uint8_t *out, size_t out_stride, uint32_t *record, int *status,
                      int *payload_bytes, int *frame_bytes)
{
    if (payload_bytes) *payload_bytes = 0;
    if (frame_bytes) *frame_bytes = 0;
    ReedCode c;
    const int rc = reed_checked(prim, fcr, step, n, n_par, depth, &c);
    if (rc != SFE_OK) return rc;
    if (encode != 0 && encode != 1) {
        set_error("reed: encode = %d is neither 0 nor 1", encode);
        return SFE_EINVAL;
    }
    const size_t P = (size_t)c.payload_bytes(), Fb = (size_t)c.frame_bytes();
    if (payload_bytes) *payload_bytes = (int)P;
    if (frame_bytes) *frame_bytes = (int)Fb;
    if (!in || n_frames == 0) return SFE_OK;
    if (n_frames >= ((size_t)1 << 31)) {
        set_error("reed: n_frames = %zu must be below 2^31", n_frames);
        return SFE_EINVAL;
    }
    const size_t in_row = encode ? P : Fb, out_row = encode ? Fb : P;
    if (in_stride < in_row || (out && out_stride < out_row)) {
        set_error("reed: in_stride %zu < the %zu bytes read per frame, or out_stride %zu < the %zu bytes written per frame", in_stride, in_row,
                  out_stride, out_row);
        return SFE_ERANGE;
    }
    for (size_t b = 0; b < n_frames; b++) {
        if (encode) {
            if (out) reed_encode_frame(c, whiten, in + b * in_stride, out + b * out_stride);
        } else {
            reed_decode_frame(c, whiten, in + b * in_stride, status_in && status_in[b] != 0, out ? out + b * out_stride : nullptr,
                              record ? record + 2 * b : nullptr, status ? status + b : nullptr);
        }
    }
    return SFE_OK;
}

int sfe_dsp_reed_create(int prim, int fcr, int step, int n, int n_par, int depth, const uint8_t *whiten, int device, sfe_reed_t *out)
{
    if (!out) return SFE_EINVAL;
    *out = nullptr;
    std::unique_ptr<Reed> p(new (std::nothrow) Reed);
    if (!p) return SFE_ENOMEM;
    int rc = reed_checked(prim, fcr, step, n, n_par, depth, &p->code);
    if (rc != SFE_OK) return rc;
    CreateScope scope(device);
    if (scope.rc != SFE_OK) return scope.rc;
    p->device = device;
    p->whiten = whiten != nullptr;
    const ReedCode &c = p->code;
    std::vector<uint8_t> tab(REED_TAB_BYTES, 0);
    std::memcpy(&tab[REED_TAB_ROOT], c.root, REED_MAX_PAR);
    std::memcpy(&tab[REED_TAB_GEN], c.gen, REED_MAX_PAR);
    std::memcpy(&tab[REED_TAB_ZINV], c.zinv, REED_MAX_N + 1);
    std::memcpy(&tab[REED_TAB_XF], c.xf, REED_MAX_N + 1);
    if (whiten) {
        const int Fb = c.frame_bytes();
        std::memcpy(&tab[REED_TAB_WHITEN], whiten, (size_t)Fb);
        for (int h = 0; h < 4; h++)
            for (int i = 0; i + h < Fb; i++) tab[REED_TAB_WHITEN4 + h * REED_WHITEN_ROW + i] = whiten[i + h];
    }
    if ((rc = p->d_tab.upload(tab)) != SFE_OK) return rc;
    *out = p.release();
    return SFE_OK;
}

int sfe_dsp_reed_encode_stream(sfe_reed_t h, const void *d_payload, size_t in_stride, size_t n_frames, void *d_frame, size_t out_stride,
                               size_t *n_out, sfe_stream_t stream)
{
    static const char who[] = "reed_encode_stream";
    Reed *p = stream_handle(as_reed(h), who, n_out);
    if (!p) return SFE_EINVAL;
    bool go;
    int rc = check_rows(who, REED_NOUNS, n_frames, d_payload, in_stride, (size_t)p->code.payload_bytes(), 1, nullptr, d_frame, out_stride,
                        (size_t)p->code.frame_bytes(), nullptr, nullptr, &go);
    if (rc != SFE_OK || !go) return rc;
    SFE_ON_DEVICE(p->device);
    ReedArgs a = reed_args(*p);
    a.in = static_cast<const uint8_t *>(d_payload);
    a.out = static_cast<uint8_t *>(d_frame);
    a.in_stride = (long long)in_stride, a.out_stride = (long long)out_stride, a.n_frames = (long long)n_frames;
    if ((rc = launch_reed_encode(a, (hipStream_t)stream)) != SFE_OK) return rc;
    *n_out = n_frames;
    return SFE_OK;
}

int sfe_dsp_reed_process_stream(sfe_reed_t h, const void *d_frame, size_t in_stride, const void *d_status_in, size_t n_frames, void *d_out,
                                size_t out_stride, void *d_rec, void *d_status, size_t *n_out, sfe_stream_t stream)
{
    static const char who[] = "reed_process_stream";
    Reed *p = stream_handle(as_reed(h), who, n_out);
    if (!p) return SFE_EINVAL;
    bool go;
    int rc = check_rows(who, REED_NOUNS, n_frames, d_frame, in_stride, (size_t)p->code.frame_bytes(), 1, d_status_in, d_out, out_stride,
                        (size_t)p->code.payload_bytes(), d_rec, d_status, &go);
    if (rc != SFE_OK || !go) return rc;
    SFE_ON_DEVICE(p->device);
    ReedArgs a = reed_args(*p);
    a.in = static_cast<const uint8_t *>(d_frame);
    a.status_in = static_cast<const int *>(d_status_in);
    a.out = static_cast<uint8_t *>(d_out);
    a.rec = static_cast<uint32_t *>(d_rec);
    a.status = static_cast<int *>(d_status);
    a.in_stride = (long long)in_stride, a.out_stride = (long long)out_stride, a.n_frames = (long long)n_frames;
    if ((rc = launch_reed_decode(a, (hipStream_t)stream)) != SFE_OK) return rc;
    *n_out = n_frames;
    return SFE_OK;
}

int sfe_dsp_reed_destroy(sfe_reed_t h) { return destroy_handle(as_reed(h)); }

}  // extern "C"
