// polar.hip -- the kernel of the FM, phase and envelope detector (sfe_dsp_polar_*, include/sfe_dsp.h): one real float32 out
// per complex sample in, by the law of polar_law.h.  Compiled with -ffp-contract=off (build.py: EXACT_SOURCES); the host
// plan (api_polar.hip) compiles the same header, and the two give the same bits.
//
// A bandwidth kernel: 12 bytes per sample (cf32) or 6 (u8) against some fifty vector instructions.  One launch per call,
// tiles x streams workgroups, no LDS, no barrier, no scratch, no atomics.
//   - A row's output starts at any 4-byte boundary, so the row is cut at the first 16-byte boundary of its OUTPUT: h = 0..3
//     head samples, then Q groups of four samples, then 0..3 tail samples.  A lane owns one group: it stores one aligned
//     16-byte vector, and loads its four samples as two 16-byte vectors where the row's input lies so (else four 8-byte
//     ones); four byte pairs are one 8-byte load (else four 2-byte ones).  Which form is chosen per row: a scalar branch.
//   - FM needs x[4t - 1] beside the group: it is the last sample of the lane below, taken by one DPP shift of the wave per
//     float (no LDS crossbar).  The first lane of a wave reads it from memory, the owner of sample 0 from the carried state.
//   - The head and the tail are peeled by a few lanes of the row's first workgroup, one sample each.
//   - Whoever owns sample n_in - 1 writes it, as float32, where the next call finds it (FM only).
// A workgroup takes POLAR_ITER runs of 256 groups one after the other, so that its loads are in flight together.
#include "polar.h"
#include "polar_law.h"

namespace sfe {
namespace {

constexpr int POLAR_THREADS = 256;
constexpr int POLAR_ITER = 4;               // runs of POLAR_THREADS groups per workgroup: a tile is 4096 samples

// lane l receives lane l - 1's value (lane 0 of the wave: 0)
__device__ __forceinline__ float wave_shr1(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x138 /* wave_shr:1 */, 0xf, 0xf, false));
}

__device__ __forceinline__ PolarC polar_pair(unsigned w) { return PolarC{polar_u8(w & 255u), polar_u8((w >> 8) & 255u)}; }

template <bool U8>
__device__ __forceinline__ PolarC polar_load(const char *row, unsigned i)
{
    if (U8) return polar_pair(*reinterpret_cast<const unsigned short *>(row + 2 * (size_t)i));
    const v2f v = *reinterpret_cast<const v2f *>(row + 8 * (size_t)i);
    return PolarC{v.x, v.y};
}

// samples i0 .. i0 + 3; wide: the address is 16-byte (cf32) or 8-byte (u8) aligned
template <bool U8>
__device__ __forceinline__ void polar_load4(const char *row, unsigned i0, bool wide, PolarC x[4])
{
    if (U8) {
        const char *p = row + 2 * (size_t)i0;
        unsigned w[4];
        if (wide) {
            const uint2 v = *reinterpret_cast<const uint2 *>(p);
            w[0] = v.x;
            w[1] = v.x >> 16;
            w[2] = v.y;
            w[3] = v.y >> 16;
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) w[k] = reinterpret_cast<const unsigned short *>(p)[k];
        }
#pragma unroll
        for (int k = 0; k < 4; k++) x[k] = polar_pair(w[k]);
    } else {
        const char *p = row + 8 * (size_t)i0;
        if (wide) {
            const v4f a = reinterpret_cast<const v4f *>(p)[0], b = reinterpret_cast<const v4f *>(p)[1];
            x[0] = PolarC{a.x, a.y};
            x[1] = PolarC{a.z, a.w};
            x[2] = PolarC{b.x, b.y};
            x[3] = PolarC{b.z, b.w};
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const v2f v = reinterpret_cast<const v2f *>(p)[k];
                x[k] = PolarC{v.x, v.y};
            }
        }
    }
}

template <int MODE, bool U8>
__global__ __launch_bounds__(POLAR_THREADS) void polar_kernel(PolarArgs a)
{
    constexpr bool FM = MODE == POLAR_FM;
    const unsigned s = blockIdx.y, n = a.n_in;
    const char *__restrict__ in = static_cast<const char *>(a.in) + (size_t)s * (size_t)a.in_stride * (U8 ? 2 : 8);
    float *__restrict__ out = a.out + (size_t)s * (size_t)a.out_stride;
    unsigned h = (unsigned)((16u - (unsigned)(reinterpret_cast<uintptr_t>(out) & 15u)) & 15u) >> 2;
    if (h > n) h = n;
    const unsigned Q = (n - h) >> 2, tail0 = h + 4 * Q;         // groups; the first tail sample
    const bool wide = ((reinterpret_cast<uintptr_t>(in) + (U8 ? 2u : 8u) * h) & (U8 ? 7u : 15u)) == 0;
    const PolarC zero{0.0f, 0.0f};

#pragma unroll
    for (int it = 0; it < POLAR_ITER; it++) {
        const unsigned t = (blockIdx.x * POLAR_ITER + it) * POLAR_THREADS + threadIdx.x;
        const bool act = t < Q;
        const unsigned i0 = h + 4 * t;
        PolarC x[4] = {zero, zero, zero, zero};
        if (act) polar_load4<U8>(in, i0, wide, x);
        PolarC p = zero;
        if (FM) {               // every lane of the wave takes part in the shift, whatever it owns
            p.r = wave_shr1(x[3].r);
            p.i = wave_shr1(x[3].i);
            if (act && (threadIdx.x & 63) == 0) {
                if (i0) p = polar_load<U8>(in, i0 - 1);
                else p = PolarC{a.state_cur[s].x, a.state_cur[s].y};
            }
        }
        if (act) {
            v4f y;
            y.x = polar_sample<MODE>(x[0], p, a.gain);
            y.y = polar_sample<MODE>(x[1], x[0], a.gain);
            y.z = polar_sample<MODE>(x[2], x[1], a.gain);
            y.w = polar_sample<MODE>(x[3], x[2], a.gain);
            *reinterpret_cast<v4f *>(out + i0) = y;
            if (FM && i0 + 3 == n - 1) a.state_nxt[s] = v2f{x[3].r, x[3].i};
        }
    }

    // the row's first workgroup also takes the head (lanes 0 .. h - 1) and the tail (lanes 64 .. ), a sample each
    if (blockIdx.x == 0) {
        const unsigned k = threadIdx.x;
        unsigned i = 0;
        bool on = false;
        if (k < h) {
            i = k;
            on = true;
        } else if (k >= 64 && k - 64 < n - tail0) {
            i = tail0 + (k - 64);
            on = true;
        }
        if (on) {
            const PolarC x = polar_load<U8>(in, i);
            PolarC p = zero;
            if (FM) {
                if (i) p = polar_load<U8>(in, i - 1);
                else p = PolarC{a.state_cur[s].x, a.state_cur[s].y};
            }
            out[i] = polar_sample<MODE>(x, p, a.gain);
            if (FM && i == n - 1) a.state_nxt[s] = v2f{x.r, x.i};
        }
    }
}

template <int MODE, bool U8>
int polar_go(const PolarArgs &a, int n_streams, hipStream_t st)
{
    constexpr unsigned per = POLAR_THREADS * POLAR_ITER;
    const unsigned groups = a.n_in >> 2, tiles = groups ? (groups + per - 1) / per : 1u;     // a row has at most n_in / 4 groups
    hipLaunchKernelGGL((polar_kernel<MODE, U8>), dim3(tiles, (unsigned)n_streams), dim3(POLAR_THREADS), 0, st, a);
    SFE_HIP(hipGetLastError());
    return SFE_OK;
}

}  // namespace

int launch_polar(int mode, int in_u8, const PolarArgs &a, int n_streams, hipStream_t st)
{
    switch (mode * 2 + (in_u8 ? 1 : 0)) {
    case 0: return polar_go<POLAR_FM, false>(a, n_streams, st);
    case 1: return polar_go<POLAR_FM, true>(a, n_streams, st);
    case 2: return polar_go<POLAR_PM, false>(a, n_streams, st);
    case 3: return polar_go<POLAR_PM, true>(a, n_streams, st);
    case 4: return polar_go<POLAR_AM, false>(a, n_streams, st);
    case 5: return polar_go<POLAR_AM, true>(a, n_streams, st);
    }
    set_error("polar: mode %d has no kernel", mode);
    return SFE_EINVAL;
}

}  // namespace sfe
