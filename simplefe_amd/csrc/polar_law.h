// polar_law.h -- the law of the FM, phase and envelope detector (sfe_dsp_polar_*, include/sfe_dsp.h), compiled twice: by
// polar.hip for the device and by api_polar.hip for sfe_dsp_polar_plan on the host.  The two must give the same bits, so
// there is nothing here for a compiler to contract: every multiply that feeds an add is an explicit fmaf, everything else
// is one IEEE float32 operation (a division and a square root that are correctly rounded on both sides), and contraction
// is switched off in every function all the same.
#pragma once
#include <math.h>

#include <hip/hip_runtime.h>

namespace sfe {

enum { POLAR_FM = 0, POLAR_PM = 1, POLAR_AM = 2 };      // SFE_POLAR_* of include/sfe_dsp.h

struct PolarC {
    float r, i;
};

constexpr float POLAR_PI_2 = 0x1.921fb6p+0f, POLAR_PI = 0x1.921fb6p+1f;
// atan(z) / z as a polynomial in z^2 on [0, 1]: a weighted least-squares fit at Chebyshev nodes
constexpr float POLAR_C0 = 0x1.fffffcp-1f, POLAR_C1 = -0x1.555390p-2f, POLAR_C2 = 0x1.995304p-3f, POLAR_C3 = -0x1.2215e6p-3f,
                POLAR_C4 = 0x1.ae613cp-4f, POLAR_C5 = -0x1.28e046p-4f, POLAR_C6 = 0x1.46db72p-5f, POLAR_C7 = -0x1.d9c858p-7f,
                POLAR_C8 = 0x1.43849ep-9f;

// one byte of the u8 wire format, exactly as sfe_dsp_rx_u8_to_f32 converts it (common.h: u8_to_f32)
__host__ __device__ inline float polar_u8(unsigned b)
{
#pragma clang fp contract(off)
    return ((float)b - 128.0f) * (1.0f / 127.0f);
}

__host__ __device__ inline float polar_at2(float y, float x)
{
#pragma clang fp contract(off)
    const float ax = fabsf(x), ay = fabsf(y);
    const float mx = fmaxf(ax, ay), mn = fminf(ax, ay);
    const float z = mx == 0.0f ? 0.0f : mn / mx;
    const float s = z * z;
    float q = POLAR_C8;
    q = fmaf(q, s, POLAR_C7);
    q = fmaf(q, s, POLAR_C6);
    q = fmaf(q, s, POLAR_C5);
    q = fmaf(q, s, POLAR_C4);
    q = fmaf(q, s, POLAR_C3);
    q = fmaf(q, s, POLAR_C2);
    q = fmaf(q, s, POLAR_C1);
    q = fmaf(q, s, POLAR_C0);
    float r = q * z;
    if (ay > ax) r = POLAR_PI_2 - r;
    if (x < 0.0f) r = POLAR_PI - r;
    if (y < 0.0f) r = -r;
    return r;
}

// y[n] of sample x whose predecessor is p (read in FM only)
template <int MODE>
__host__ __device__ inline float polar_sample(PolarC x, PolarC p, float gain)
{
#pragma clang fp contract(off)
    if (MODE == POLAR_FM) {
        const float re = fmaf(x.r, p.r, x.i * p.i);
        const float im = fmaf(x.i, p.r, -(x.r * p.i));
        return gain * polar_at2(im, re);
    }
    if (MODE == POLAR_PM) return gain * polar_at2(x.i, x.r);
    return gain * sqrtf(fmaf(x.r, x.r, x.i * x.i));
}

}  // namespace sfe
