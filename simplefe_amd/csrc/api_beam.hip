// api_beam.hip -- the beamformer handle behind sfe_beam_t, sfe_dsp_beam_* (include/sfe_dsp.h).  Host code only; the
// kernels are in beam.hip.  What the kernels multiply by is computed here: each band's real matrix, every entry formed
// in float64 from the float32 weights and rounded once, then laid out in the order the kernel's lanes read it.
#include <cmath>

#include "host.h"
#include "block.h"
#include "beam.h"
#include "beam_view.h"

namespace sfe {
namespace {

struct Beam {
    static constexpr uint32_t MAGIC = 0x42454d31u;   // 'BEM1'
    uint32_t magic = MAGIC;
    int S = 0, B = 0, M = 1, device = 0, in_u8 = 0;
    DevBuf<float> d_frag;           // [M][beam_frag_floats(S, B)]
};

Beam *as_beam(void *h) { return as_handle<Beam>(h, "beamformer"); }

int beam_check(int S, int B, int M, const float *w, const float *v)
{
    if (S < 1 || S > BEAM_MAX_IN) {
        set_error("beam: n_in = %d must be in [1, %d]", S, BEAM_MAX_IN);
        return SFE_EINVAL;
    }
    if (B < 1 || B > BEAM_MAX_BEAMS) {
        set_error("beam: n_beams = %d must be in [1, %d]", B, BEAM_MAX_BEAMS);
        return SFE_EINVAL;
    }
    if (M < 1 || M > BEAM_MAX_BANDS) {
        set_error("beam: n_bands = %d must be in [1, %d]", M, BEAM_MAX_BANDS);
        return SFE_EINVAL;
    }
    if ((long long)M * B * S > BEAM_MAX_WEIGHTS) {
        set_error("beam: n_bands n_beams n_in = %lld must be at most 2^20", (long long)M * B * S);
        return SFE_EINVAL;
    }
    if (!w) {
        set_error("beam: null weights");
        return SFE_EINVAL;
    }
    const size_t nf = (size_t)M * B * S * 2;
    for (size_t i = 0; i < nf; i++)
        if (!std::isfinite(w[i]) || (v && !std::isfinite(v[i]))) {
            set_error("beam: %s weight %zu (band %zu) is not finite", std::isfinite(w[i]) ? "conjugate" : "direct", i / 2,
                      i / 2 / ((size_t)B * S));
            return SFE_EINVAL;
        }
    return SFE_OK;
}

// R_k of every band, [M][2B][2S] row-major.  Without V the entries are W's own floats up to sign.
void beam_real_matrix(int S, int B, int M, const float *w, const float *v, float *R)
{
    const size_t n2 = 2 * (size_t)S;
    for (size_t k = 0; k < (size_t)M; k++)
        for (size_t b = 0; b < (size_t)B; b++)
            for (size_t s = 0; s < (size_t)S; s++) {
                const size_t at = ((k * B + b) * S + s) * 2;
                float *r0 = R + (k * 2 * B + 2 * b) * n2 + 2 * s, *r1 = r0 + n2;
                if (!v) {
                    r0[0] = w[at];
                    r0[1] = -w[at + 1];
                    r1[0] = w[at + 1];
                    r1[1] = w[at];
                } else {
                    const double wr = w[at], wi = w[at + 1], vr = v[at], vi = v[at + 1];
                    r0[0] = (float)(wr + vr);
                    r0[1] = (float)(-wi + vi);
                    r1[0] = (float)(wi + vi);
                    r1[1] = (float)(wr - vr);
                }
            }
}

// the same matrices in the kernel's fragment order (beam.h), zero-padded to the shape's class
std::vector<float> beam_frags(int S, int B, int M, const float *w, const float *v)
{
    std::vector<float> R((size_t)M * 4 * B * S);
    beam_real_matrix(S, B, M, w, v, R.data());
    const int KS = 2 * beam_kp(S), RT = beam_rt(B);
    const size_t nf = beam_frag_floats(S, B);
    std::vector<float> f(nf * M, 0.0f);
    for (size_t k = 0; k < (size_t)M; k++)
        for (int rt = 0; rt < RT; rt++)
            for (int ks = 0; ks < KS; ks++)
                for (int lane = 0; lane < 64; lane++) {
                    int row, col;
                    beam_frag_at(rt, ks, lane, &row, &col);
                    if (row < 2 * B && col < 2 * S) f[k * nf + ((size_t)rt * KS + ks) * 64 + lane] = R[(k * 2 * B + row) * 2 * S + col];
                }
    return f;
}

}  // namespace

bool beam_view(void *h, BeamView *out)
{
    Beam *p = as_beam(h);
    if (!p) return false;
    *out = BeamView{p->S, p->B, p->M, p->device, p->d_frag};
    return true;
}

}  // namespace sfe

using namespace sfe;

extern "C" {

int sfe_dsp_beam_plan(int n_in, int n_beams, int n_bands, const float *weights, const float *weights_conj, float *real_matrix)
{
    const int rc = beam_check(n_in, n_beams, n_bands, weights, weights_conj);
    if (rc != SFE_OK) return rc;
    if (real_matrix) beam_real_matrix(n_in, n_beams, n_bands, weights, weights_conj, real_matrix);
    return SFE_OK;
}

int sfe_dsp_beam_create(const float *weights, const float *weights_conj, int n_in, int n_beams, int n_bands, int device,
                        sfe_beam_t *out)
{
    if (!out) return SFE_EINVAL;
    *out = nullptr;
    int rc = beam_check(n_in, n_beams, n_bands, weights, weights_conj);
    if (rc != SFE_OK) return rc;
    CreateScope scope(device);
    if (scope.rc != SFE_OK) return scope.rc;
    std::unique_ptr<Beam> p(new (std::nothrow) Beam);
    if (!p) return SFE_ENOMEM;
    p->S = n_in;
    p->B = n_beams;
    p->M = n_bands;
    p->device = device;
    if ((rc = p->d_frag.upload(beam_frags(n_in, n_beams, n_bands, weights, weights_conj))) != SFE_OK) return rc;
    SFE_HIP(hipDeviceSynchronize());
    *out = p.release();
    return SFE_OK;
}

int sfe_dsp_beam_set_input_format(sfe_beam_t h, int fmt)
{
    return set_format(as_beam(h), "beam_set_input_format", fmt, SFE_FMT_U8, "SFE_FMT_U8", &Beam::in_u8);
}

int sfe_dsp_beam_set_weights(sfe_beam_t h, const float *weights, const float *weights_conj)
{
    Beam *p = as_beam(h);
    if (!p) return SFE_EINVAL;
    const int rc = beam_check(p->S, p->B, p->M, weights, weights_conj);
    if (rc != SFE_OK) return rc;
    const std::vector<float> f = beam_frags(p->S, p->B, p->M, weights, weights_conj);
    SFE_ON_DEVICE(p->device);
    // calls already enqueued read the table: they finish with the old one before it is replaced
    SFE_HIP(hipDeviceSynchronize());
    SFE_HIP(hipMemcpy(p->d_frag, f.data(), f.size() * sizeof(float), hipMemcpyHostToDevice));
    SFE_HIP(hipDeviceSynchronize());
    return SFE_OK;
}

int sfe_dsp_beam_process_stream(sfe_beam_t h, const void *d_in, size_t n_in, size_t in_stride, void *d_out, size_t out_stride,
                                size_t *n_out, sfe_stream_t stream)
{
    static const char who[] = "beam_process_stream";
    Beam *p = stream_handle(as_beam(h), who, n_out);
    if (!p) return SFE_EINVAL;
    static const StreamNouns nouns{"n_in = ", "cf32 8 B, u8 (I,Q) pairs 2 B", true, false};
    bool go;
    int rc = check_streams(who, nouns, d_in, n_in, in_stride, (size_t)p->S * p->M, p->in_u8 ? 2 : 8, d_out, out_stride, n_in,
                           (size_t)p->B * p->M, sizeof(v2f), &go);
    if (rc != SFE_OK || !go) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (stream_is_capturing(s)) {       // set_weights may replace the table a captured call would have pinned
        set_error("beam_process_stream: graph capture is not supported (set_weights may replace the weight table)");
        return SFE_ESTATE;
    }
    SFE_ON_DEVICE(p->device);
    rc = launch_beam(p->in_u8, d_in, (long long)in_stride, static_cast<v2f *>(d_out), (long long)out_stride, p->d_frag,
                     (long long)n_in, p->S, p->B, p->M, s);
    if (rc != SFE_OK) return rc;
    *n_out = n_in;
    return SFE_OK;
}

int sfe_dsp_beam_destroy(sfe_beam_t h) { return destroy_handle(as_beam(h)); }

}  // extern "C"
