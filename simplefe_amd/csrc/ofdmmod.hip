// ofdmmod.hip -- OFDM burst modulator (sfe_dsp_ofdmmod_*): per burst, a row of coded bits or of cf32 symbols becomes one
// frame of T training and Ns data symbols, each N samples behind its cyclic prefix, at a stated place of an output stream,
// cf32 or the 10-bit transmit wire format; every sample of the stream in no frame is written as +0 by the same launch
// (include/sfe_dsp.h states the law; ofdmmod_law.h is the law operation by operation, compiled here and by the host plan,
// whose bits these are).
//
// ONE WORKGROUP PER (BURST, SYMBOL) -- no estimate is shared between the symbols of a burst, so nothing orders them -- of
// ofdm_threads(log2 N) lanes, and one workgroup per tile of OFDMMOD_ZTILE samples in no frame.  The grid is the tiles of
// the zeros before the first frame, then per burst its T + Ns symbols followed by the tiles of the gap up to the next frame,
// then the tiles behind the last frame: every sample, and under TX10 every 5-byte group, is written by exactly one workgroup.
//   bins    lane t fills V[t], V[t + NT], ... in LDS through the bin list made at create (om_bin): a table value, a pilot
//           times the symbol's sign, +0, or the data bin's one or two bits / its cf32 symbol, read where the row lies.
//   passes  one radix-2 pass when log2 N is odd, then radix-4 Stockham passes, in place in LDS with ofdm.hip's barrier
//           pattern: every lane reads its butterflies, barrier, writes them, barrier.  The butterflies are om_butterfly's.
//   store   frame sample m of the symbol is V[(m + N - cp) mod N] / N: the tail as prefix, then the body, in one run of
//           coalesced stores.  cf32: a lane stores two neighbouring samples as 16 bytes from the first 16-byte boundary
//           on (the sample in front of it, where there is one, goes alone).  TX10: a lane owns a group; cp, start_base and
//           start_step are even, so a symbol and every run of zeros is whole groups.
// No atomics, no scratch, nothing carried.  Explicit fmaf only (the file is compiled without contraction).
#include "ofdmmod.h"

namespace sfe {

namespace {

template <int LOGN, int R>
__device__ __forceinline__ void ofdmmod_pass(omc *V, const omc *tw, int logLs, int tid)
{
    constexpr int N = 1 << LOGN, NT = ofdm_threads(LOGN), NQ = N / R, NI = NQ < NT ? 1 : NQ / NT;
    static_assert(NQ < NT || NI * NT == NQ, "whole passes per lane");
    const int Ls = 1 << logLs;
    omc y[NI][R];
#pragma unroll
    for (int e = 0; e < NI; e++) {
        const int j = e * NT + tid;
        if (NQ >= NT || j < NQ) {
#pragma unroll
            for (int r = 0; r < R; r++) y[e][r] = V[j + r * NQ];
            om_butterfly<R>(LOGN, logLs, j, tw, y[e]);
        }
    }
    lds_barrier();
#pragma unroll
    for (int e = 0; e < NI; e++) {
        const int j = e * NT + tid;
        if (NQ >= NT || j < NQ) {
            const int base = om_out_base<R>(logLs, j);
#pragma unroll
            for (int r = 0; r < R; r++) V[base + r * Ls] = y[e][r];
        }
    }
    lds_barrier();
}

// samples [A0, A0 + cnt) of the stream, sample A0 + m being get(m); under TX10 A0 and cnt are even
template <int NT, bool TX10, class G>
__device__ __forceinline__ void ofdmmod_put(void *out, long long A0, int cnt, int tid, G get)
{
    if constexpr (TX10) {
        unsigned char *p = static_cast<unsigned char *>(out) + (A0 >> 1) * 5;
        for (int m = 2 * tid; m < cnt; m += 2 * NT) {
            uint32_t w;
            uint8_t last;
            om_group(get(m), get(m + 1), &w, &last);
            unsigned char *q = p + (m >> 1) * 5;
            __builtin_memcpy(q, &w, 4);
            q[4] = last;
        }
    } else {
        omc *p = static_cast<omc *>(out) + A0;
        const int odd = (int)((reinterpret_cast<uintptr_t>(p) >> 3) & 1u);
        if (odd && tid == 0 && cnt > 0) p[0] = get(0);
        for (int m = odd + 2 * tid; m < cnt; m += 2 * NT) {
            const omc y0 = get(m);
            if (m + 1 < cnt) {
                const omc y1 = get(m + 1);
                *reinterpret_cast<v4f *>(p + m) = v4f{y0.x, y0.y, y1.x, y1.y};
            } else {
                p[m] = y0;
            }
        }
    }
}

template <int LOGN, bool TX10>
__global__ __launch_bounds__(ofdm_threads(LOGN)) void ofdmmod_kernel(OfdmmodArgs a)
{
    constexpr int N = 1 << LOGN, NT = ofdm_threads(LOGN), NE = N / NT;
    __shared__ omc V[N];
    const int tid = (int)threadIdx.x;
    const OmodLaw &law = a.law;
    const int nsym = law.T + law.Ns, cp = law.cp, L = N + cp;
    const long long B = blockIdx.x, nb = a.n_bursts, per_burst = nsym + a.gap_tiles, step = nb > 1 ? a.start_step : 0;

    // ---- a run of zeros [Z0, Z1), or a symbol
    long long Z0, Z1;
    if (B < a.n_lead) {
        Z0 = B * OFDMMOD_ZTILE;
        Z1 = min(Z0 + OFDMMOD_ZTILE, nb ? a.start_base : a.n_out);
    } else if (B < a.n_lead + nb * per_burst) {
        const long long e = B - a.n_lead, burst = e / per_burst, o = a.start_base + burst * step;
        const int r = (int)(e - burst * per_burst);
        if (r < nsym) {
            const void *row = law.symbols ? static_cast<const void *>(static_cast<const omc *>(a.in) + burst * a.in_stride)
                                          : static_cast<const void *>(static_cast<const uint8_t *>(a.in) + burst * a.in_stride);
#pragma unroll
            for (int e2 = 0; e2 < NE; e2++) {
                const int k = e2 * NT + tid;
                V[k] = om_bin(law, row, r, k);
            }
            lds_barrier();
            int logLs = 0;
            if constexpr (LOGN & 1) {
                ofdmmod_pass<LOGN, 2>(V, law.tw, 0, tid);
                logLs = 1;
            }
#pragma unroll
            for (; logLs < LOGN; logLs += 2) ofdmmod_pass<LOGN, 4>(V, law.tw, logLs, tid);
            const float inv_n = 1.0f / (float)N;
            ofdmmod_put<NT, TX10>(a.out, o + (long long)r * L, L, tid, [&](int m) { return om_scale(V[om_frame_src(m, N, cp)], inv_n); });
            return;
        }
        const long long len = burst == nb - 1 ? (long long)a.F : a.start_step, s0 = a.F + (long long)(r - nsym) * OFDMMOD_ZTILE;
        if (s0 >= len) return;                                  // the last burst's slot is its frame
        Z0 = o + s0;
        Z1 = o + min(s0 + OFDMMOD_ZTILE, len);
    } else {
        Z0 = a.start_base + (nb - 1) * step + a.F + (B - a.n_lead - nb * per_burst) * OFDMMOD_ZTILE;
        Z1 = min(Z0 + OFDMMOD_ZTILE, a.n_out);
    }
    if (Z1 > Z0) ofdmmod_put<NT, TX10>(a.out, Z0, (int)(Z1 - Z0), tid, [](int) { return omc{0.0f, 0.0f}; });
}

template <int LOGN>
int ofdmmod_launch_n(const OfdmmodArgs &a, const dim3 &grid, hipStream_t st)
{
    const dim3 block(ofdm_threads(LOGN));
    if (a.tx10) hipLaunchKernelGGL((ofdmmod_kernel<LOGN, true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((ofdmmod_kernel<LOGN, false>), grid, block, 0, st, a);
    SFE_HIP(hipGetLastError());
    return SFE_OK;
}

}  // namespace

int launch_ofdmmod(const OfdmmodArgs &a, long long n_wg, hipStream_t st)
{
    if (n_wg <= 0) return SFE_OK;
    const dim3 grid((unsigned)n_wg);
    switch (a.law.logn) {
    case 6: return ofdmmod_launch_n<6>(a, grid, st);
    case 7: return ofdmmod_launch_n<7>(a, grid, st);
    case 8: return ofdmmod_launch_n<8>(a, grid, st);
    case 9: return ofdmmod_launch_n<9>(a, grid, st);
    case 10: return ofdmmod_launch_n<10>(a, grid, st);
    case 11: return ofdmmod_launch_n<11>(a, grid, st);
    case 12: return ofdmmod_launch_n<12>(a, grid, st);
    }
    set_error("ofdmmod: log2 N = %d has no kernel", a.law.logn);
    return SFE_EINVAL;
}

}  // namespace sfe
