// burst.hip -- feed-forward burst demodulator (sfe_dsp_burst_*): per (stream, burst) a window of the stream that starts
// where the correlator's peak says becomes N symbol-rate samples, timing-, frequency-, phase- and amplitude-corrected,
// with a record of the estimates (include/sfe_dsp.h states the law; api_burst.hip is its float64 twin).
//
// ONE WORKGROUP (256 lanes) PER BURST, nothing carried, no atomics.
//   gate     the gate value, the start offset and the range of the reach are the same words for every lane: a gated or
//            out-of-range burst stores its zeros, its record and its status and leaves before a sample is read.
//   pass 1   the reach of (N + 2) sps samples, lanes along the samples (coalesced): the finite check, the copy into LDS
//            where the reach fits (burst.h: a slot of padding per symbol period of an even sps), and the Oerder-Meyr sum of |x|^2 against the table of sps
//            twiddles, which sits in LDS -- no sine or cosine per sample.
//   y        lanes along the symbols: four samples sps apart per lane from LDS (the padding of burst.h keeps a half-wave
//            on 32 different bank pairs) or, above the threshold, from global memory a second time (through L2); y and, over the
//            preamble, z = y conj(p) stay in LDS.
//   sums     c, then R, then S (with the energy of y over the preamble beside it), then the error of the preamble: each
//            a strided chain of explicit multiply-adds per lane, a six-step butterfly inside the wave (the same bits in
//            every lane) and ((w0 + w1) + w2) + w3 across the four waves through LDS.
//   phase    the turn count theta + f k is formed and reduced in float64 -- the one use of float64 -- and only the
//            reduced turn, at most half a turn, goes to float32 and to sinpif / cospif.
// The order of every sum is a function of (sps, N, Lp, lag) alone: never of the burst, the stream, an address or a stride.
#include <cfloat>

#include "burst.h"

namespace sfe {

namespace {

__device__ inline float wave_sum(float v)      // the same bits in all 64 lanes; every lane of the wave must be active
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = v + __shfl_xor(v, m);
    return v;
}

// v[0..NV) summed over the workgroup, the same bits in every lane; every lane must be here
template <int NV>
__device__ inline void block_sum(float (&v)[NV], float *red, int lane, int wave)
{
#pragma unroll
    for (int i = 0; i < NV; i++) {
        v[i] = wave_sum(v[i]);
        if (lane == 0) red[wave * 4 + i] = v[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; i++) v[i] = ((red[i] + red[4 + i]) + red[8 + i]) + red[12 + i];
    __syncthreads();
}

template <bool U8>
__device__ inline v2f load_in(const void *base, long long i)
{
    if (U8) {
        const unsigned w = static_cast<const uint16_t *>(base)[i];
        return v2f{u8_to_f32(w & 0xffu), u8_to_f32(w >> 8)};
    }
    return static_cast<const v2f *>(base)[i];
}

__device__ inline bool finite32(float v) { return fabsf(v) <= FLT_MAX; }

// exp(-j 2 pi t) for a turn count formed in float64: reduced there, evaluated in float32
__device__ inline v2f unturn(double t)
{
    const float r = (float)(t - rint(t));
    return v2f{cospif(2.0f * r), -sinpif(2.0f * r)};
}

template <bool U8>
__global__ __launch_bounds__(256) void burst_kernel(BurstArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sps = a.sps, N = a.N, Lp = a.Lp, lag = a.lag, pad = burst_pad(sps);
    v2f *y = reinterpret_cast<v2f *>(smem), *z = y + N, *tw = z + Lp;       // [N], [Lp], [64]
    float *red = reinterpret_cast<float *>(tw + BURST_MAX_SPS);             // [4][4]
    v2f *xs = reinterpret_cast<v2f *>(red + BURST_RED_WORDS);               // the reach, padded (staged launches only)
    const long long blk = blockIdx.x, s = blk / a.n_bursts, b = blk - s * a.n_bursts;
    v2f *out = a.out + blk * a.out_stride;
    float *rec = a.rec ? a.rec + blk * BURST_REC : nullptr;
    int *stat = a.status ? a.status + s * a.status_stride + b : nullptr;
    const float qnan = __builtin_nanf("");

    // what a burst without an answer gets: N symbols of +0, a record of NaN (its last two words +0), its status
    auto fail = [&](int st) {
        for (int k = tid; k < N; k += 256) out[k] = v2f{0.0f, 0.0f};
        if (rec && tid < BURST_REC) rec[tid] = tid < 6 ? qnan : 0.0f;
        if (stat && tid == 0) *stat = st;
    };

    // ---- gate and range: the same words in every lane
    if (a.gate && !(a.gate[s * a.gate_stride + b] >= a.min_gate)) return fail(BURST_GATED);
    const long long o = a.start_base + b * a.start_step + (a.idx ? (long long)a.idx[s * a.idx_stride + b] : 0LL);
    const int reach = (N + 2) * sps;
    if (o < sps || o - sps > a.n_in - reach) return fail(BURST_OUT_OF_RANGE);
    const long long x0 = s * a.in_stride + o - sps;         // sample 0 of the reach

    if (tid < sps) tw[tid] = a.tw[tid];
    __syncthreads();

    // ---- pass 1: finite check, staging, timing sum
    float c[2] = {0.0f, 0.0f};
    int bad = 0;
    {
        int r = tid % sps, sym = tid / sps;                  // i = sym sps + r, carried by addition
        const int rstep = 256 % sps, symstep = 256 / sps;
        for (int i = tid; i < reach; i += 256) {
            const v2f v = load_in<U8>(a.in, x0 + i);
            bad |= !(finite32(v.x) && finite32(v.y));
            if (a.staged) xs[i + sym * pad] = v;
            if (!a.fixed_timing && i >= sps && i < reach - sps) {
                const float p = fmaf(v.y, v.y, v.x * v.x);
                const v2f w = tw[r];
                c[0] = fmaf(p, w.x, c[0]);
                c[1] = fmaf(p, w.y, c[1]);
            }
            r += rstep, sym += symstep;
            if (r >= sps) r -= sps, sym++;
        }
    }
    bad = __syncthreads_or(bad);        // also: the staged reach is complete
    float tau = 0.0f;
    if (!a.fixed_timing) {
        block_sum(c, red, lane, wave);
        if (!(finite32(c[0]) && finite32(c[1])) || (c[0] == 0.0f && c[1] == 0.0f)) return fail(BURST_NO_ESTIMATE);
        const float t = fminf(fmaxf(atan2f(c[1], c[0]) / 6.2831855f, -0.5f), 0.5f);
        tau = 0.0f - (float)sps * t;
        if (tau <= -0.5f * (float)sps) tau += (float)sps;
    }
    if (bad) return fail(BURST_NO_ESTIMATE);

    // ---- interpolate: y[k], and over the preamble z[k] = y[k] conj(p[k]) and the energy of y
    const int m = (int)floorf(tau);
    const float mu = tau - (float)m;
    const float L[4] = {(-mu * (mu - 1.0f) * (mu - 2.0f)) / 6.0f, ((mu + 1.0f) * (mu - 1.0f) * (mu - 2.0f)) / 2.0f,
                        (-(mu + 1.0f) * mu * (mu - 2.0f)) / 2.0f, ((mu + 1.0f) * mu * (mu - 1.0f)) / 6.0f};
    float sv[3] = {0.0f, 0.0f, 0.0f};                       // S (re, im), sum |y|^2 over the preamble
    for (int k = tid; k < N; k += 256) {
        const int i0 = sps + k * sps + m - 1;               // in [sps/2 - 1, reach - sps/2 + 1]: inside the reach
        float yr = 0.0f, yi = 0.0f;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int d = m - 1 + q, e = d < 0 ? -1 : (d >= sps ? 1 : 0);       // sample i0 + q lies in symbol period k + 1 + e
            const v2f v = a.staged ? xs[i0 + q + (k + 1 + e) * pad] : load_in<U8>(a.in, x0 + i0 + q);
            yr = fmaf(L[q], v.x, yr);
            yi = fmaf(L[q], v.y, yi);
        }
        y[k] = v2f{yr, yi};
        if (k < Lp) {
            const v2f p = a.pre[k];
            z[k] = v2f{fmaf(yr, p.x, yi * p.y), fmaf(yi, p.x, -(yr * p.y))};
            sv[2] = fmaf(yi, yi, fmaf(yr, yr, sv[2]));
        }
    }
    __syncthreads();

    // ---- carrier frequency: R = sum z[k + lag] conj(z[k])
    float R[2] = {0.0f, 0.0f};
    for (int k = tid; k < Lp - lag; k += 256) {
        const v2f u = z[k + lag], v = z[k];
        R[0] = fmaf(u.x, v.x, fmaf(u.y, v.y, R[0]));
        R[1] = fmaf(u.y, v.x, fmaf(-u.x, v.y, R[1]));
    }
    block_sum(R, red, lane, wave);
    if (!(finite32(R[0]) && finite32(R[1])) || (R[0] == 0.0f && R[1] == 0.0f)) return fail(BURST_NO_ESTIMATE);
    const float f = atan2f(R[1], R[0]) / (6.2831855f * (float)lag);

    // ---- phase and amplitude: S = sum z[k] exp(-j 2 pi f k)
    for (int k = tid; k < Lp; k += 256) {
        const v2f e = unturn((double)f * (double)k), v = z[k];
        sv[0] = fmaf(v.x, e.x, fmaf(-v.y, e.y, sv[0]));
        sv[1] = fmaf(v.y, e.x, fmaf(v.x, e.y, sv[1]));
    }
    block_sum(sv, red, lane, wave);
    const float S2 = fmaf(sv[1], sv[1], sv[0] * sv[0]);
    const float amp = sqrtf(S2) / a.E_p;
    if (!(finite32(sv[0]) && finite32(sv[1])) || (sv[0] == 0.0f && sv[1] == 0.0f) || !(amp > 0.0f) || !finite32(amp))
        return fail(BURST_NO_ESTIMATE);
    const float theta = atan2f(sv[1], sv[0]) / 6.2831855f;

    // ---- output, and the error over the preamble
    float ev[1] = {0.0f};
    for (int k = tid; k < N; k += 256) {
        const v2f e = unturn((double)theta + (double)f * (double)k), v = y[k];
        const v2f w = v2f{fmaf(v.x, e.x, -(v.y * e.y)) / amp, fmaf(v.y, e.x, v.x * e.y) / amp};
        out[k] = w;
        if (k < Lp) {
            const v2f p = a.pre[k];
            const float dr = w.x - p.x, di = w.y - p.y;
            ev[0] = fmaf(di, di, fmaf(dr, dr, ev[0]));
        }
    }
    block_sum(ev, red, lane, wave);
    if (rec && tid == 0) {
        rec[0] = tau, rec[1] = f, rec[2] = theta, rec[3] = amp;
        rec[4] = S2 / (a.E_p * sv[2]);
        rec[5] = ev[0] / a.E_p;
        rec[6] = rec[7] = 0.0f;
    }
    if (stat && tid == 0) *stat = BURST_OK;
}

}  // namespace

int launch_burst(const BurstArgs &a, int in_u8, int n_streams, hipStream_t st)
{
    const dim3 grid((unsigned)(a.n_bursts * n_streams));
    const size_t lds = burst_base_bytes(a.N, a.Lp) + (a.staged ? burst_stage_bytes(a.sps, a.N) : 0);
    if (in_u8) {
        if (lds > 65536) SFE_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&burst_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(burst_kernel<true>, grid, dim3(256), lds, st, a);
    } else {
        if (lds > 65536) SFE_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&burst_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(burst_kernel<false>, grid, dim3(256), lds, st, a);
    }
    SFE_HIP(hipGetLastError());
    return SFE_OK;
}

}  // namespace sfe
