// api_polar.hip -- the detector handle behind sfe_polar_t, sfe_dsp_polar_* (include/sfe_dsp.h), and the host plan.  Host code
// only; the kernel is polar.hip, the law both run is polar_law.h.
#include <cmath>
#include <cstring>

#include "host.h"
#include "block.h"
#include "polar.h"
#include "polar_law.h"

namespace sfe {
namespace {

struct Polar {
    static constexpr uint32_t MAGIC = 0x504f4c31u;   // 'POL1'
    uint32_t magic = MAGIC;
    int mode = 0, n_streams = 1, device = 0, in_u8 = 0;
    float gain = 1.0f;
    CarriedPair state;              // per stream x[-1] of the next call as (re, im) float32 (FM)
    bool captured = false;          // a hipGraph names state.cur(): the state stays there for good (CarriedPair::carry)
};

Polar *as_polar(void *h) { return as_handle<Polar>(h, "detector"); }

int polar_check(int mode, float gain)
{
    if (mode != SFE_POLAR_FM && mode != SFE_POLAR_PM && mode != SFE_POLAR_AM) {
        set_error("polar: mode = %d is none of SFE_POLAR_FM, SFE_POLAR_PM, SFE_POLAR_AM", mode);
        return SFE_EINVAL;
    }
    if (!std::isfinite(gain)) {
        set_error("polar: gain is not finite");
        return SFE_EINVAL;
    }
    return SFE_OK;
}

int polar_check_fmt(int fmt)
{
    if (fmt == SFE_FMT_F32 || fmt == SFE_FMT_U8) return SFE_OK;
    set_error("polar: input format %d is neither SFE_FMT_F32 nor SFE_FMT_U8", fmt);
    return SFE_EINVAL;
}

template <int MODE>
void polar_run(float gain, bool u8, const void *in, size_t n, PolarC *prev, float *out)
{
    const unsigned char *b = static_cast<const unsigned char *>(in);
    PolarC p = *prev;
    for (size_t i = 0; i < n; i++) {
        PolarC x;
        if (u8) {
            x = PolarC{polar_u8(b[2 * i]), polar_u8(b[2 * i + 1])};
        } else {
            float v[2];
            memcpy(v, b + 8 * i, sizeof(v));        // any alignment
            x = PolarC{v[0], v[1]};
        }
        out[i] = polar_sample<MODE>(x, p, gain);
        p = x;
    }
    *prev = p;
}

}  // namespace
}  // namespace sfe

using namespace sfe;

extern "C" {

int sfe_dsp_polar_plan(int mode, float gain, int fmt, const void *in, size_t n_in, float prev[2], float *out)
{
    int rc = polar_check(mode, gain);
    if (rc != SFE_OK || (rc = polar_check_fmt(fmt)) != SFE_OK) return rc;
    if (n_in == 0) return SFE_OK;
    if (!in || !out) {
        set_error("polar: null buffer");
        return SFE_EINVAL;
    }
    PolarC p = prev ? PolarC{prev[0], prev[1]} : PolarC{0.0f, 0.0f};
    const bool u8 = fmt == SFE_FMT_U8;
    if (mode == SFE_POLAR_FM) polar_run<POLAR_FM>(gain, u8, in, n_in, &p, out);
    else if (mode == SFE_POLAR_PM) polar_run<POLAR_PM>(gain, u8, in, n_in, &p, out);
    else polar_run<POLAR_AM>(gain, u8, in, n_in, &p, out);
    if (prev) {
        prev[0] = p.r;
        prev[1] = p.i;
    }
    return SFE_OK;
}

int sfe_dsp_polar_create(int mode, float gain, int n_streams, int device, sfe_polar_t *out)
{
    if (!out) return SFE_EINVAL;
    *out = nullptr;
    int rc = polar_check(mode, gain);
    if (rc != SFE_OK) return rc;
    if (n_streams < 1 || n_streams > POLAR_MAX_STREAMS) {
        set_error("polar: n_streams = %d must be in [1, %d]", n_streams, POLAR_MAX_STREAMS);
        return SFE_EINVAL;
    }
    CreateScope scope(device);
    if (scope.rc != SFE_OK) return scope.rc;
    std::unique_ptr<Polar> p(new (std::nothrow) Polar);
    if (!p) return SFE_ENOMEM;
    p->mode = mode;
    p->gain = gain;
    p->n_streams = n_streams;
    p->device = device;
    if ((rc = p->state.alloc_zero((size_t)n_streams * sizeof(v2f))) != SFE_OK) return rc;
    SFE_HIP(hipDeviceSynchronize());
    *out = p.release();
    return SFE_OK;
}

int sfe_dsp_polar_set_input_format(sfe_polar_t h, int fmt)
{
    Polar *p = as_polar(h);
    if (!p) {
        set_error("polar: set_input_format on a null handle");
        return SFE_EINVAL;
    }
    const int rc = polar_check_fmt(fmt);
    if (rc != SFE_OK) return rc;
    p->in_u8 = fmt == SFE_FMT_U8;
    return SFE_OK;
}

int sfe_dsp_polar_process_stream(sfe_polar_t h, const void *d_in, size_t n_in, size_t in_stride, float *d_out, size_t out_stride,
                                 size_t *n_out, sfe_stream_t stream)
{
    static const char who[] = "polar_process_stream";
    Polar *p = stream_handle(as_polar(h), who, n_out);
    if (!p) return SFE_EINVAL;
    static const StreamNouns nouns{"n_in = ", "cf32 8 B, u8 (I,Q) pairs 2 B, float32 4 B", true, true};
    bool go;
    int rc = check_streams(who, nouns, d_in, n_in, in_stride, p->n_streams, p->in_u8 ? 2 : 8, d_out, out_stride, n_in, p->n_streams,
                           sizeof(float), &go);
    if (rc != SFE_OK || !go) return rc;
    hipStream_t s = (hipStream_t)stream;
    SFE_ON_DEVICE(p->device);
    const bool fm = p->mode == SFE_POLAR_FM;
    if (fm && stream_is_capturing(s)) p->captured = true;
    PolarArgs a;
    a.in = d_in;
    a.out = d_out;
    a.state_cur = p->state.cur<v2f>();
    a.state_nxt = p->state.next<v2f>();
    a.in_stride = (long long)in_stride;
    a.out_stride = (long long)out_stride;
    a.n_in = (unsigned)n_in;
    a.gain = p->gain;
    rc = launch_polar(p->mode, p->in_u8, a, p->n_streams, s);
    if (rc != SFE_OK) return rc;
    // phase and envelope carry nothing; FM's last sample is where the next call, or the next replay, looks for it
    if (fm && (rc = p->state.carry(p->captured, s)) != SFE_OK) return rc;
    *n_out = n_in;
    return SFE_OK;
}

int sfe_dsp_polar_reset(sfe_polar_t h)
{
    Polar *p = as_polar(h);
    if (!p) return SFE_EINVAL;
    return reset_pairs(p->device, {&p->state});
}

int sfe_dsp_polar_destroy(sfe_polar_t h) { return destroy_handle(as_polar(h)); }

}  // extern "C"
