// mod.hip -- burst modulator (sfe_dsp_mod_*): per burst, ceil(n_info / 8) packed payload bytes become one pulse-shaped
// frame of complex baseband samples at a stated place of an output stream, cf32 or the 10-bit transmit wire format; every
// sample of the stream in no frame is written as +0 by the same launch (include/sfe_dsp.h states the law; api_mod.hip is
// its host twin, whose bits these are).
//
// ONE WORKGROUP PER TILE of MOD_TILE consecutive samples.  The tiles partition the stream: the zeros before the first
// frame, then each burst's slot [o_b, o_b + start_step) cut from o_b on -- the last burst's slot ends with its frame --
// then the zeros behind the last frame.  A tile therefore lies in one burst's slot or in no frame at all.
//   stage   the taps, zero-filled up to Q sps, and the symbols the tile's samples read -- symbol floor(f0 / sps) - (Q - 1)
//           to symbol floor((f1 - 1) / sps), the halo derived again by every tile, nothing carried -- as float2 in LDS.  A
//           thread per symbol: a preamble symbol is read from the handle's table; a data symbol's one or two coded bits
//           come straight from at most two payload bytes each -- the code is feed-forward, so coded bit (t, j) is
//           parity(reg_t & g_j) with reg_t the K payload bits that end at t -- and the table of a period's kept positions
//           that travels with the launch says which (t, j) coded bit i is.
//   barrier one.
//   sum     a thread takes two neighbouring samples at a time; sample f = k sps + r is the fmaf chain from +0 over
//           q = 0 .. Q - 1 of h[q sps + r] s[k - q], the terms whose symbol lies outside [0, N) left out.  Neighbouring lanes
//           read neighbouring taps and (mostly) the same symbol.
//   store   cf32: 16 bytes per thread where the pair's address allows it, else two 8-byte stores.  TX10: a thread owns the
//           5-byte group of an EVEN sample of the stream and its successor; groups are aligned to the stream, not to
//           frames or tiles, so the successor of a tile's last sample may lie in the next tile, in the next burst's frame
//           or in no frame: that one sample per tile is summed straight from global memory by the same functions.
// No atomics, no scratch.  Explicit fmaf only (the file is compiled without contraction): the bits are the host plan's.
#include "mod.h"

namespace sfe {

namespace {

// the shift register of step t: bit i is payload bit t - i (0 before the payload and behind it), i < K
__device__ inline unsigned mod_reg(const ModArgs &a, const uint8_t *row, int t)
{
    const int m = t >> 3, nbytes = (a.n_info + 7) >> 3;
    const unsigned lo = m < nbytes ? row[m] : 0u, hi = (m >= 1 && m - 1 < nbytes) ? row[m - 1] : 0u;
    unsigned reg = ((hi << 8) | lo) >> (7 - (t & 7));           // payload bit t in bit 0, MSB-first bytes
    if (t >= a.n_info) reg &= ~((1u << (t - a.n_info + 1)) - 1u);   // the termination tail, and the last byte's pad bits
    return reg & ((1u << a.K) - 1u);
}

// coded bit i of the burst, i < n_soft
__device__ inline unsigned mod_coded_bit(const ModArgs &a, const uint8_t *row, int i)
{
    if (a.n_gen == 0) return ((unsigned)row[i >> 3] >> (7 - (i & 7))) & 1u;
    const int per = i / a.per_period;
    const unsigned e = a.pos[i - per * a.per_period];
    const int t = per * a.P + (int)(e >> 2);
    return (unsigned)__popc(mod_reg(a, row, t) & a.gen[e & 3u]) & 1u;
}

// symbol k of the burst, 0 <= k < N
__device__ inline v2f mod_symbol(const ModArgs &a, const uint8_t *row, int k)
{
    if (k < a.Lp) return a.pre[k];
    const int i = k - a.Lp;
    if (a.order == 2) return v2f{mod_coded_bit(a, row, i) ? -a.a : a.a, 0.0f};
    const unsigned c0 = mod_coded_bit(a, row, 2 * i), c1 = 2 * i + 1 < a.n_soft ? mod_coded_bit(a, row, 2 * i + 1) : 0u;
    return v2f{c0 ? -a.a : a.a, c1 ? -a.a : a.a};
}

// Sample i of the stream, 0 <= i < n_out, from global memory alone: the successor of a tile's last sample under TX10.
__device__ v2f mod_sample_of_stream(const ModArgs &a, long long i)
{
    v2f acc = v2f{0.0f, 0.0f};
    if (a.n_bursts == 0 || i < a.start_base) return acc;
    const long long rel = i - a.start_base;
    long long b = a.n_bursts > 1 ? rel / a.start_step : 0;
    if (b > a.n_bursts - 1) b = a.n_bursts - 1;
    const long long f = rel - b * (a.n_bursts > 1 ? a.start_step : 0);
    if (f >= a.F) return acc;
    const uint8_t *row = a.bytes + b * a.in_stride;
    const int k = (int)f / a.sps, r = (int)f - k * a.sps;
    for (int q = 0; q < a.Q && q <= k; q++) {
        const int kk = k - q, t = q * a.sps + r;
        if (kk >= a.N || t >= a.n_taps) continue;
        const float h = a.taps[t];
        const v2f s = mod_symbol(a, row, kk);
        acc.x = fmaf(h, s.x, acc.x);
        acc.y = fmaf(h, s.y, acc.y);
    }
    return acc;
}

template <bool TX10>
__global__ __launch_bounds__(MOD_THREADS) void mod_kernel(ModArgs a)
{
    __shared__ float h[MOD_MAX_TAPS];
    __shared__ v2f sym[MOD_TILE_SYMS];
    const int tid = (int)threadIdx.x;
    const long long B = blockIdx.x, nb = a.n_bursts, slot_tiles = nb * a.tiles_per_slot;

    // ---- the tile: samples [A0, A1) of the stream; in a burst's slot, frame samples [f0, f1) of it are inside the frame
    long long A0, A1, o = 0, burst = 0;
    int f0 = 0, f1 = 0;
    if (B < a.n_lead) {
        A0 = B * MOD_TILE;
        A1 = min(A0 + MOD_TILE, nb ? a.start_base : a.n_out);
    } else if (B < a.n_lead + slot_tiles) {
        const long long e = B - a.n_lead;
        burst = e / a.tiles_per_slot;
        const long long s0 = (e - burst * a.tiles_per_slot) * MOD_TILE, len = burst == nb - 1 ? (long long)a.F : a.start_step;
        if (s0 >= len) return;                                  // the last burst's slot is its frame: fewer tiles
        const long long s1 = min(s0 + MOD_TILE, len);
        o = a.start_base + burst * (nb > 1 ? a.start_step : 0);
        A0 = o + s0, A1 = o + s1;
        if (s0 < a.F) f0 = (int)s0, f1 = (int)min(s1, (long long)a.F);
    } else {
        A0 = a.start_base + (nb - 1) * (nb > 1 ? a.start_step : 0) + a.F + (B - a.n_lead - slot_tiles) * MOD_TILE;
        A1 = min(A0 + MOD_TILE, a.n_out);
    }
    const bool framed = f1 > f0;
    const int sps = a.sps, Q = a.Q, N = a.N;

    // ---- stage the taps and the tile's symbols
    int klo = 0;
    if (framed) {
        for (int i = tid; i < Q * sps; i += MOD_THREADS) h[i] = i < a.n_taps ? a.taps[i] : 0.0f;
        klo = f0 / sps - (Q - 1);
        const int n_sym = (f1 - 1) / sps - klo + 1;             // <= (MOD_TILE - 1) / sps + 1 + Q <= MOD_TILE_SYMS
        const uint8_t *row = a.bytes + burst * a.in_stride;
        for (int i = tid; i < n_sym; i += MOD_THREADS) {
            const int k = klo + i;
            sym[i] = (k >= 0 && k < N) ? mod_symbol(a, row, k) : v2f{0.0f, 0.0f};
        }
    }
    __syncthreads();

    // sample i of the tile, A0 <= i < A1
    auto sample = [&](long long i) {
        v2f acc = v2f{0.0f, 0.0f};
        const long long fl = i - o;
        if (!framed || fl >= f1) return acc;                    // behind the frame, or in no frame
        const int f = (int)fl, k = f / sps, r = f - k * sps;
        const int q0 = max(0, k - N + 1), q1 = min(Q - 1, k);
        for (int q = q0; q <= q1; q++) {
            const float hv = h[q * sps + r];
            const v2f s = sym[k - q - klo];
            acc.x = fmaf(hv, s.x, acc.x);
            acc.y = fmaf(hv, s.y, acc.y);
        }
        return acc;
    };

    // ---- pairs of neighbouring samples; under TX10 a pair is a group of the stream and starts on an even sample
    const long long S0 = TX10 ? A0 + (A0 & 1) : A0;
    for (long long i0 = S0 + 2 * tid; i0 < A1; i0 += 2 * MOD_THREADS) {
        const long long i1 = i0 + 1;
        const v2f y0 = sample(i0);
        const bool two = i1 < A1;
        const v2f y1 = two ? sample(i1) : (TX10 ? mod_sample_of_stream(a, i1) : v2f{0.0f, 0.0f});
        mod_store_pair<TX10>(a.out, i0, y0, y1, two);
    }
}

}  // namespace

int launch_mod(const ModArgs &a, long long n_tiles, hipStream_t st)
{
    if (n_tiles <= 0) return SFE_OK;
    if (a.tx10) hipLaunchKernelGGL(mod_kernel<true>, dim3((unsigned)n_tiles), dim3(MOD_THREADS), 0, st, a);
    else hipLaunchKernelGGL(mod_kernel<false>, dim3((unsigned)n_tiles), dim3(MOD_THREADS), 0, st, a);
    SFE_HIP(hipGetLastError());
    return SFE_OK;
}

}  // namespace sfe
