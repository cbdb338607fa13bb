// ofdm.hip -- OFDM burst receiver (sfe_dsp_ofdm_*): per (stream, burst) a reach of T training and Ns data symbols that
// starts where the correlator's peak says becomes Ns rows of Nd equalised data-bin symbols, a channel estimate H[N], a
// record and a status (include/sfe_dsp.h states the law; api_ofdm.hip is its float64 twin).
//
// ONE WORKGROUP PER BURST (ofdm.h: N / 4 lanes, 64 to 256), nothing carried, no atomics, no split of a burst: the order
// of every sum is a function of the shape alone -- never of the burst, the stream, an address or a stride.
//   gate     the gate value, the start offset and the range of the reach are the same words for every lane: a gated or
//            out-of-range burst stores its zeros, its record and its status and leaves, the whole workgroup together,
//            before a sample is read and before the first barrier.
//   pass 1   the reach, symbol by symbol, lanes along the samples (coalesced): the finite check, and over the prefixes
//            from cfo_skip on the products with the sample N later (a second read, through L2) for gamma.
//   H        T transforms in LDS; lane t owns bins t, t + NT, ...: their sum, times the table c, stays in LDS as N cf32.
//            h2 and the smallest |H|^2 are workgroup reductions.
//   symbol   load with the rotation (the turn count eps n / N is formed and reduced in float64 -- the one use of
//            float64 -- and only the reduced turn goes to float32 and to sinpif / cospif), one radix-2 pass when log2 N is
//            odd, radix-4 Stockham passes as psd.hip lays them into LDS (twiddles from the table made at create), the
//            pilot sum P_j over the list of pilot bins, phi_j, the pilot error, and the data bins through the list of
//            data bins: lane i writes symbol i, one coalesced store of Nd cf32.
// From pass 1 on a burst that has failed (status 1) keeps running to every barrier with the others: what it computes is
// discarded at the end, where the same lanes that wrote its symbols write their zeros.  No index depends on a sample.
#include <cfloat>

#include "fft16.h"
#include "ofdm.h"

namespace sfe {

namespace {

__device__ inline float wave_sum(float v)      // the same bits in all 64 lanes; every lane of the wave must be active
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = v + __shfl_xor(v, m);
    return v;
}

__device__ inline float wave_min(float v)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = fminf(v, __shfl_xor(v, m));
    return v;
}

// v[0..NV) summed (MIN: the smallest) over the workgroup of NT lanes, the same bits in every lane; every lane must be here
template <int NT, bool MIN, int NV>
__device__ inline void block_fold(float (&v)[NV], float *red, int lane, int wave)
{
    constexpr int NW = NT / 64;
    static_assert(NV <= OFDM_RED_WORDS / 4, "a row of red per wave");
#pragma unroll
    for (int i = 0; i < NV; i++) {
        v[i] = MIN ? wave_min(v[i]) : wave_sum(v[i]);
        if (NW > 1 && lane == 0) red[wave * (OFDM_RED_WORDS / 4) + i] = v[i];
    }
    if constexpr (NW > 1) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NV; i++) {
            float r = red[i];
#pragma unroll
            for (int w = 1; w < NW; w++) r = MIN ? fminf(r, red[w * (OFDM_RED_WORDS / 4) + i]) : r + red[w * (OFDM_RED_WORDS / 4) + i];
            v[i] = r;
        }
        __syncthreads();
    }
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

__device__ inline v2f mul(v2f a, v2f b) { return v2f{fmaf(a.x, b.x, -(a.y * b.y)), fmaf(a.y, b.x, a.x * b.y)}; }          // a b
__device__ inline v2f mul_conj(v2f a, v2f b) { return v2f{fmaf(a.x, b.x, a.y * b.y), fmaf(a.y, b.x, -(a.x * b.y))}; }     // a conj(b)

// one forward Stockham pass of radix R over the N values in LDS: sub-transforms of length Ls = 2^logLs become R Ls long
template <int LOGN, int R>
__device__ __forceinline__ void ofdm_pass(v2f *V, const v2f *tw, int logLs, int tid)
{
    constexpr int N = 1 << LOGN, NT = ofdm_threads(LOGN), NQ = N / R, NI = NQ < NT ? 1 : NQ / NT, LOGR = R == 4 ? 2 : 1;
    static_assert(NQ < NT || NI * NT == NQ, "whole passes per lane");
    const int Ls = 1 << logLs;
    v2f y[NI][R];
#pragma unroll
    for (int e = 0; e < NI; e++) {
        const int j = e * NT + tid, k = j & (Ls - 1);
        if (NQ >= NT || j < NQ) {
            v2f x[R];
#pragma unroll
            for (int r = 0; r < R; r++) x[r] = V[j + r * NQ];
            if (logLs > 0) {
#pragma unroll
                for (int r = 1; r < R; r++) x[r] = cmul(x[r], tw[(r * k) << (LOGN - logLs - LOGR)]);
            }
            if constexpr (R == 4) {
                const v2f t0 = x[0] + x[2], t1 = x[0] - x[2], t2 = x[1] + x[3], t3 = x[1] - x[3];
                y[e][0] = t0 + t2;
                y[e][1] = add_mj(t1, t3);       // x0 - j x1 - x2 + j x3
                y[e][2] = t0 - t2;
                y[e][3] = add_pj(t1, t3);
            } else {
                y[e][0] = x[0] + x[1];
                y[e][1] = x[0] - x[1];
            }
        }
    }
    lds_barrier();
#pragma unroll
    for (int e = 0; e < NI; e++) {
        const int j = e * NT + tid, k = j & (Ls - 1);
        const int base = ((j >> logLs) << (logLs + LOGR)) + k;
        if (NQ >= NT || j < NQ) {
#pragma unroll
            for (int r = 0; r < R; r++) V[base + r * Ls] = y[e][r];
        }
    }
    lds_barrier();
}

template <int LOGN, bool U8>
__global__ __launch_bounds__(ofdm_threads(LOGN)) void ofdm_kernel(OfdmArgs a)
{
    constexpr int N = 1 << LOGN, NT = ofdm_threads(LOGN), NE = N / NT;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    v2f *V = reinterpret_cast<v2f *>(smem), *Hs = V + N;        // [N], [N]
    float *red = reinterpret_cast<float *>(Hs + N);             // [4][8]
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int L = N + a.cp, nsym = a.T + a.Ns, Nd = a.Nd, Np = a.Np;
    const long long blk = blockIdx.x, s = blk / a.n_bursts, b = blk - s * a.n_bursts;
    v2f *out = a.out + blk * a.out_stride;
    v2f *chan = a.chan ? a.chan + blk * N : nullptr;
    float *rec = a.rec ? a.rec + blk * OFDM_REC : nullptr;
    int *stat = a.status ? a.status + s * a.status_stride + b : nullptr;
    const float qnan = __builtin_nanf("");

    // what a burst without an answer gets: Ns Nd symbols of +0 (lane i writes symbol i of every row, as the output loop
    // does), a row of H of +0, a record of NaN (its last two words +0), its status
    auto fail = [&](int st) {
        for (int j = 0; j < a.Ns; j++)
            for (int i = tid; i < Nd; i += NT) out[(long long)j * Nd + i] = v2f{0.0f, 0.0f};
        if (chan)
            for (int k = tid; k < N; k += NT) chan[k] = v2f{0.0f, 0.0f};
        if (rec && tid < OFDM_REC) rec[tid] = tid < 6 ? qnan : 0.0f;
        if (stat && tid == 0) *stat = st;
    };

    // ---- gate and range: the same words in every lane
    if (a.gate && !(a.gate[s * a.gate_stride + b] >= a.min_gate)) return fail(OFDM_GATED);
    const long long o = a.start_base + b * a.start_step + (a.idx ? (long long)a.idx[s * a.idx_stride + b] : 0LL);
    const long long reach = (long long)nsym * L;                // below 2^31 (create)
    if (o < 0 || o > a.n_in - reach) return fail(OFDM_OUT_OF_RANGE);
    const long long x0 = s * a.in_stride + o;                   // sample 0 of the reach

    // ---- pass 1: finite check, gamma over the prefixes
    int bad = 0;
    float gm[2] = {0.0f, 0.0f};
    for (int j = 0; j < nsym; j++) {
        const long long base = x0 + (long long)j * L;
        for (int i = tid; i < L; i += NT) {
            const v2f v = load_in<U8>(a.in, base + i);
            bad |= !(finite32(v.x) && finite32(v.y));
            if (a.cfo && i >= a.q && i < a.cp) {
                const v2f u = load_in<U8>(a.in, base + i + N);          // i + N < L: inside the symbol
                gm[0] = fmaf(u.x, v.x, fmaf(u.y, v.y, gm[0]));
                gm[1] = fmaf(u.y, v.x, fmaf(-u.x, v.y, gm[1]));
            }
        }
    }
    float eps = 0.0f;
    if (a.cfo) {
        block_fold<NT, false>(gm, red, lane, wave);
        if (!(finite32(gm[0]) && finite32(gm[1])) || (gm[0] == 0.0f && gm[1] == 0.0f)) bad = 1;
        eps = fminf(fmaxf(atan2f(gm[1], gm[0]) / 6.2831855f, -0.5f), 0.5f);
    }

    // symbol j's window, rotated, into V, and its transform; V is whole and visible to every lane on return
    const double inv_n = 1.0 / (double)N;
    auto transform = [&](int j) {
        const int n0 = j * L + a.cp - a.g;                      // the window's first sample, counted from o
#pragma unroll
        for (int e = 0; e < NE; e++) {
            const int m = e * NT + tid;
            v2f v = load_in<U8>(a.in, x0 + n0 + m);
            if (a.cfo) v = mul(v, unturn((double)eps * (double)(n0 + m) * inv_n));
            V[m] = v;
        }
        lds_barrier();
        int logLs = 0;
        if constexpr (LOGN & 1) {
            ofdm_pass<LOGN, 2>(V, a.tw, 0, tid);
            logLs = 1;
        }
#pragma unroll
        for (; logLs < LOGN; logLs += 2) ofdm_pass<LOGN, 4>(V, a.tw, logLs, tid);
    };

    // ---- channel: lane t owns bins t + e NT, in V (the load and the last pass leave bin k with the lane that owns it
    // only after a barrier, which transform ends with) and in Hs
    v2f hacc[NE];
#pragma unroll
    for (int e = 0; e < NE; e++) hacc[e] = v2f{0.0f, 0.0f};
    for (int j = 0; j < a.T; j++) {
        transform(j);
#pragma unroll
        for (int e = 0; e < NE; e++) hacc[e] = hacc[e] + V[e * NT + tid];
        lds_barrier();                                          // the next load writes V
    }
    float hs[1] = {0.0f}, hm[1] = {FLT_MAX};
#pragma unroll
    for (int e = 0; e < NE; e++) {
        const int k = e * NT + tid;
        const v2f c = a.c[k];
        const bool used = c.x != 0.0f || c.y != 0.0f;
        const v2f h = used ? mul(hacc[e], c) : v2f{0.0f, 0.0f};
        Hs[k] = h;
        if (used) {
            const float p = fmaf(h.y, h.y, h.x * h.x);
            bad |= !(p > 0.0f && finite32(p));
            hs[0] = hs[0] + p;
            hm[0] = fminf(hm[0], p);
        }
    }
    block_fold<NT, false>(hs, red, lane, wave);
    block_fold<NT, true>(hm, red, lane, wave);
    bad = __syncthreads_or(bad);                                // also: Hs is whole
    const float h2 = hs[0] / a.nu;

    // ---- the data symbols
    float perr[1] = {0.0f}, a0 = 0.0f, a1 = 0.0f;
    for (int j = 0; j < a.Ns; j++) {
        transform(a.T + j);
        v2f phi = v2f{1.0f, 0.0f};
        if (Np > 0) {
            const float sg = a.sign[j];
            float P[2] = {0.0f, 0.0f};
            for (int i = tid; i < Np; i += NT) {
                const int k = a.bins[Nd + i];
                const v2f hp = mul(Hs[k], a.pilot[k]) * v2f{sg, sg}, y = V[k];
                P[0] = fmaf(y.x, hp.x, fmaf(y.y, hp.y, P[0]));
                P[1] = fmaf(y.y, hp.x, fmaf(-y.x, hp.y, P[1]));
            }
            block_fold<NT, false>(P, red, lane, wave);
            const float mag = hypotf(P[0], P[1]);
            if (!(finite32(P[0]) && finite32(P[1])) || !(mag > 0.0f) || !finite32(mag)) bad = 1;        // the same bits in every lane
            phi = v2f{P[0] / mag, P[1] / mag};
            for (int i = tid; i < Np; i += NT) {
                const int k = a.bins[Nd + i];
                const v2f h = Hs[k], z = mul_conj(V[k], mul(h, phi)), p = a.pilot[k];
                const float den = fmaf(h.y, h.y, h.x * h.x), dr = z.x / den - p.x * sg, di = z.y / den - p.y * sg;
                perr[0] = fmaf(di, di, fmaf(dr, dr, perr[0]));
            }
        }
        if (j == 0) a0 = atan2f(phi.y, phi.x) / 6.2831855f;
        if (j == a.Ns - 1) a1 = atan2f(phi.y, phi.x) / 6.2831855f;
        v2f *row = out + (long long)j * Nd;
        for (int i = tid; i < Nd; i += NT) {
            const int k = a.bins[i];
            const v2f h = Hs[k], z = mul_conj(V[k], mul(h, phi));
            const float den = a.mrc ? h2 : fmaf(h.y, h.y, h.x * h.x);
            row[i] = v2f{z.x / den, z.y / den};
        }
        lds_barrier();                                          // the next load writes V
    }
    if (Np > 0) block_fold<NT, false>(perr, red, lane, wave);

    if (bad) return fail(OFDM_NO_ESTIMATE);
    if (chan)
        for (int k = tid; k < N; k += NT) chan[k] = Hs[k];
    if (rec && tid == 0) {
        rec[0] = eps, rec[1] = h2, rec[2] = hm[0] / h2;
        rec[3] = Np > 0 ? perr[0] / a.pilot_den : 0.0f;
        rec[4] = a0, rec[5] = a1;
        rec[6] = rec[7] = 0.0f;
    }
    if (stat && tid == 0) *stat = OFDM_OK;
}

template <int LOGN>
int ofdm_launch_n(const OfdmArgs &a, int in_u8, const dim3 &grid, hipStream_t st)
{
    const dim3 block(ofdm_threads(LOGN));
    if (in_u8) hipLaunchKernelGGL((ofdm_kernel<LOGN, true>), grid, block, ofdm_lds_bytes(LOGN), st, a);
    else hipLaunchKernelGGL((ofdm_kernel<LOGN, false>), grid, block, ofdm_lds_bytes(LOGN), st, a);
    SFE_HIP(hipGetLastError());
    return SFE_OK;
}

template <int LOGN>
int ofdm_prepare_n()
{
    const int lds = (int)ofdm_lds_bytes(LOGN);
    SFE_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&ofdm_kernel<LOGN, true>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    SFE_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&ofdm_kernel<LOGN, false>), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    return SFE_OK;
}

}  // namespace

int ofdm_prepare(int logn)
{
    if (ofdm_lds_bytes(logn) <= 65536) return SFE_OK;
    return logn == 12 ? ofdm_prepare_n<12>() : SFE_EINVAL;      // N = 4096 alone passes 64 KiB
}

int launch_ofdm(const OfdmArgs &a, int in_u8, int n_streams, hipStream_t st)
{
    const dim3 grid((unsigned)(a.n_bursts * n_streams));
    switch (a.logn) {
    case 6: return ofdm_launch_n<6>(a, in_u8, grid, st);
    case 7: return ofdm_launch_n<7>(a, in_u8, grid, st);
    case 8: return ofdm_launch_n<8>(a, in_u8, grid, st);
    case 9: return ofdm_launch_n<9>(a, in_u8, grid, st);
    case 10: return ofdm_launch_n<10>(a, in_u8, grid, st);
    case 11: return ofdm_launch_n<11>(a, in_u8, grid, st);
    case 12: return ofdm_launch_n<12>(a, in_u8, grid, st);
    }
    set_error("ofdm: log2 N = %d has no kernel", a.logn);
    return SFE_EINVAL;
}

}  // namespace sfe
