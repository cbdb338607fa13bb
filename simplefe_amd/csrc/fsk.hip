// fsk.hip -- the 2-(G)FSK burst modem (sfe_dsp_fsk_*), both directions (include/sfe_dsp.h states the law; fsk_law.h is
// the law, compiled here and by api_fsk.hip, whose plan's bits these are).
//
// fsk_mod_kernel<TX10>: ONE WORKGROUP PER TILE of FSK_TILE consecutive samples of the output stream, the tiles cut as
// mod.hip cuts them, so a tile lies in one burst's slot or in no frame at all.
//   count   the phase is an exact integer, so a tile needs no scan over samples: a symbol whose pulse has passed contributes
//           a_k Gsum, and the sum of the kp0 levels passed before the tile is kp0 - 2 ones, ones the count of set bits among
//           the burst's first kp0 -- preamble bytes from the handle, payload bytes from the call, at most 4 KiB through L2, a
//           byte per lane, a butterfly inside the wave and the four waves through LDS.
//   stage   the table C[0 .. n_taps] and the levels of the symbols kp0 .. floor((f1 - 1) / sps) into LDS; wave 0 forms the
//           prefix sums of those levels (a run per lane, one scan across the lanes).
//   sample  a lane forms P[i] = Gsum (A0 + prefix) + the at most Q terms in flight (fsk_law.h: fsk_phase), then fsk_cis and
//           one product per component; two neighbouring samples per lane, stored by mod.h's store path.  Under TX10 the
//           successor of a tile's last sample belongs to the tile's last group: inside the same frame it is staged with the
//           tile; otherwise it is a frame's first sample, whose phase is 0, or lies in no frame.
// fsk_demod_kernel<U8>: ONE WORKGROUP PER BURST, nothing carried, no atomics.
//   gate    as burst.hip: a gated or out-of-range burst stores its fill and leaves before a sample is read.
//   finite  the reach once, lanes along the samples (cf32 only: a byte is always finite).
//   fit     the Lp (2R + 1) preamble values of u, as many timing candidates at a time as the two trees in LDS hold; each
//           value is a lane's own chain of n_mf fmaf over the discriminator of x read through L2; the trees run in place
//           in the stride form of fsk_law.h, a barrier per level; every lane then walks the candidates' nums in order.
//   output  a lane per data symbol, its own n_mf-long chain; the packed bits are a wave's ballot, eight lanes to a byte.
// Neither v nor u of the whole reach is staged.  The order of every sum is a function of the handle alone.
#include <cfloat>

#include "fsk.h"
#include "mod.h"

namespace sfe {

namespace {

__device__ inline int wave_sum_i(int v)        // the same word in all 64 lanes; every lane of the wave must be active
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
    return v;
}

// ones among the first n bits of row, counted a byte per lane; this lane's share
__device__ inline int ones_share(const uint8_t *row, int n, int tid)
{
    int c = 0;
    for (int j = tid; 8 * j < n; j += FSK_THREADS) {
        unsigned b = row[j];
        const int rem = n - 8 * j;
        if (rem < 8) b &= (0xFFu << (8 - rem)) & 0xFFu;
        c += __popc(b);
    }
    return c;
}

// Sample i of the stream where it is not a sample of the tile's own frame: the successor of a tile's last sample under TX10.
// It is a frame's first sample -- P[0] = 0 -- or lies in no frame.
__device__ inline v2f fsk_outside(const FskModArgs &a, long long i)
{
    if (a.n_bursts == 0 || i < a.start_base) return v2f{0.0f, 0.0f};
    const long long rel = i - a.start_base;
    long long b = a.n_bursts > 1 ? rel / a.start_step : 0;
    if (b > a.n_bursts - 1) b = a.n_bursts - 1;
    if (rel - b * (a.n_bursts > 1 ? a.start_step : 0) != 0) return v2f{0.0f, 0.0f};
    const FskC y = fsk_mod_sample(0u, a.amp);
    return v2f{y.r, y.i};
}

template <bool TX10>
__global__ __launch_bounds__(FSK_THREADS) void fsk_mod_kernel(FskModArgs a)
{
    __shared__ uint32_t C[FSK_MAX_TAPS + 1];
    __shared__ int lev[FSK_TILE_SYMS];
    __shared__ int pref[FSK_TILE_SYMS + 1];
    __shared__ int red[4];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long B = blockIdx.x, nb = a.n_bursts, slot_tiles = nb * a.tiles_per_slot;

    // ---- the tile: samples [A0, A1) of the stream; in a burst's slot, frame samples [f0, f1) of it are inside the frame
    long long A0, A1, o = 0, burst = 0;
    int f0 = 0, f1 = 0;
    if (B < a.n_lead) {
        A0 = B * FSK_TILE;
        A1 = min(A0 + FSK_TILE, nb ? a.start_base : a.n_out);
    } else if (B < a.n_lead + slot_tiles) {
        const long long e = B - a.n_lead;
        burst = e / a.tiles_per_slot;
        const long long s0 = (e - burst * a.tiles_per_slot) * FSK_TILE, len = burst == nb - 1 ? (long long)a.F : a.start_step;
        if (s0 >= len) return;                                  // the last burst's slot is its frame: fewer tiles
        const long long s1 = min(s0 + FSK_TILE, len);
        o = a.start_base + burst * (nb > 1 ? a.start_step : 0);
        A0 = o + s0, A1 = o + s1;
        if (s0 < a.F) f0 = (int)s0, f1 = (int)min(s1, (long long)a.F);
    } else {
        A0 = a.start_base + (nb - 1) * (nb > 1 ? a.start_step : 0) + a.F + (B - a.n_lead - slot_tiles) * FSK_TILE;
        A1 = min(A0 + FSK_TILE, a.n_out);
    }
    const bool framed = f1 > f0;
    const int sps = a.sps, N = a.N, Lp = a.Lp, n_taps = a.n_taps;
    // under TX10 the last group's second sample may be the frame's next one: staged with the tile
    const int f1x = (TX10 && framed && f1 < a.F && o + f1 == A1) ? f1 + 1 : f1;

    // ---- count, stage, prefix
    int kp0 = 0, n_sym = 0, A_0 = 0;
    if (framed) {
        const uint8_t *row = a.bytes + burst * a.in_stride;
        kp0 = fsk_passed(f0, sps, n_taps, N);
        n_sym = max(min((f1x - 1) / sps, N - 1) - kp0 + 1, 0);      // <= FSK_TILE_SYMS (fsk.h)
        int ones = wave_sum_i(ones_share(a.pre, min(kp0, Lp), tid) + ones_share(row, max(kp0 - Lp, 0), tid));
        if (lane == 0) red[wave] = ones;
        for (int i = tid; i <= n_taps; i += FSK_THREADS) C[i] = a.C[i];
        for (int i = tid; i < n_sym; i += FSK_THREADS) {
            const int k = kp0 + i;
            lev[i] = 1 - 2 * (int)(k < Lp ? fsk_bit(a.pre, k) : fsk_bit(row, k - Lp));
        }
    }
    __syncthreads();
    if (framed) {
        A_0 = kp0 - 2 * (((red[0] + red[1]) + red[2]) + red[3]);
        if (wave == 0) {        // exclusive prefix sums of lev[0 .. n_sym), the total in pref[n_sym]
            const int chunk = (n_sym + 63) / 64, j0 = min(lane * chunk, n_sym), j1 = min(j0 + chunk, n_sym);
            int local = 0;
            for (int j = j0; j < j1; j++) local += lev[j];
            int incl = local;
#pragma unroll
            for (int m = 1; m < 64; m <<= 1) {
                const int t = __shfl_up(incl, m);
                if (lane >= m) incl += t;
            }
            int run = incl - local;
            for (int j = j0; j < j1; j++) {
                pref[j] = run;
                run += lev[j];
            }
            const int total = __shfl(incl, 63);
            if (lane == 0) pref[n_sym] = total;
        }
    }
    __syncthreads();

    // sample i of the stream, A0 <= i <= A1 (A1 itself: the successor of the tile's last sample under TX10)
    auto sample = [&](long long i) {
        const long long fl = i - o;
        if (framed && fl >= f0 && fl < f1x) {
            const int f = (int)fl, kp = fsk_passed(f, sps, n_taps, N);
            const uint32_t p = fsk_phase(f, sps, N, a.Gsum, A_0 + pref[kp - kp0], kp, C, [&](int k) { return lev[k - kp0]; });
            const FskC y = fsk_mod_sample(p, a.amp);
            return v2f{y.r, y.i};
        }
        if (i >= A1) return fsk_outside(a, i);
        return v2f{0.0f, 0.0f};                                 // behind the frame, or in no frame
    };

    // ---- pairs of neighbouring samples; under TX10 a pair is a group of the stream and starts on an even sample
    const long long S0 = TX10 ? A0 + (A0 & 1) : A0;
    for (long long i0 = S0 + 2 * tid; i0 < A1; i0 += 2 * FSK_THREADS) {
        const long long i1 = i0 + 1;
        const bool two = i1 < A1;
        const v2f y0 = sample(i0);
        const v2f y1 = (two || TX10) ? sample(i1) : v2f{0.0f, 0.0f};
        mod_store_pair<TX10>(a.out, i0, y0, y1, two);
    }
}

template <bool U8>
__global__ __launch_bounds__(FSK_THREADS) void fsk_demod_kernel(FskDemodArgs a)
{
    __shared__ float t1[FSK_TREE_WORDS], te[FSK_TREE_WORDS];
    __shared__ float cnum[FSK_CAND_WORDS], cs1[FSK_CAND_WORDS];
    __shared__ int flag;
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int sps = a.sps, N = a.N, Lp = a.Lp, n_mf = a.n_mf, R = a.R, n_bits = N - Lp;
    const long long blk = blockIdx.x, s = blk / a.n_bursts, b = blk - s * a.n_bursts;
    float *soft = a.soft + blk * a.soft_stride;
    uint8_t *bits = a.bits ? a.bits + blk * a.bits_stride : nullptr;
    float *rec = a.rec ? a.rec + blk * FSK_REC : nullptr;
    int *stat = a.status ? a.status + s * a.status_stride + b : nullptr;
    const float qnan = __builtin_nanf("");

    // what a burst without an answer gets: soft values of +0, bytes of 0, a record of NaN (its last four words +0), its status
    auto fail = [&](int st) {
        for (int t = tid; t < n_bits; t += FSK_THREADS) soft[t] = 0.0f;
        if (bits)
            for (int t = tid; t < (n_bits + 7) / 8; t += FSK_THREADS) bits[t] = 0;
        if (rec && tid < FSK_REC) rec[tid] = tid < 4 ? qnan : 0.0f;
        if (stat && tid == 0) *stat = st;
    };

    // ---- gate and range: the same words in every lane
    if (a.gate && !(a.gate[s * a.gate_stride + b] >= a.min_gate)) return fail(FSK_GATED);
    const long long o = a.start_base + b * a.start_step + (a.idx ? (long long)a.idx[s * a.idx_stride + b] : 0LL);
    const long long lo = o + a.delay - R - 1, hi = o + a.delay + R + (long long)(N - 1) * sps + n_mf;
    if (lo < 0 || hi > a.n_in) return fail(FSK_OUT_OF_RANGE);
    const long long x0 = s * a.in_stride + o;                   // sample 0 of the burst
    auto at = [&](long long n) {
        if (U8) {
            const unsigned w = static_cast<const uint16_t *>(a.in)[x0 + n];
            return PolarC{polar_u8(w & 0xffu), polar_u8(w >> 8)};
        }
        const v2f v = static_cast<const v2f *>(a.in)[x0 + n];
        return PolarC{v.x, v.y};
    };

    // ---- a non-finite sample anywhere in the reach
    if (!U8) {
        if (tid == 0) flag = 0;
        __syncthreads();
        int bad = 0;
        for (long long i = lo + tid; i < hi; i += FSK_THREADS) {
            const PolarC v = at(i - o);
            bad |= !(fabsf(v.r) <= FLT_MAX && fabsf(v.i) <= FLT_MAX);
        }
        if (bad) flag = 1;           // every writer writes the same word
        __syncthreads();
        if (flag) return fail(FSK_NO_ESTIMATE);
    }

    // the tree over every candidate's Lp2 words at once: pairs (2h k, 2h k + h); Lp2 is a multiple of 2h
    auto trees = [&](int words, int Lp2, bool both) {
        for (int h = 1; h < Lp2; h <<= 1) {
            for (int w = tid; w < words / (2 * h); w += FSK_THREADS) {
                const int i = w * 2 * h;
                t1[i] = t1[i] + t1[i + h];
                if (both) te[i] = te[i] + te[i + h];
            }
            __syncthreads();
        }
    };

    // ---- timing: the candidates tau = -R .. R, cand at a time
    const int Lp2 = fsk_pow2(Lp), cand = FSK_TREE_WORDS / Lp2, n_cand = 2 * R + 1;
    bool have = false;
    float best = 0.0f, best_S1 = 0.0f;
    int tau = 0;
    for (int c0 = 0; c0 < n_cand; c0 += cand) {
        const int nc = min(cand, n_cand - c0);
        for (int w = tid; w < nc * Lp2; w += FSK_THREADS) {
            const int c = w / Lp2, k = w - c * Lp2;
            float u = 0.0f, eu = 0.0f;
            if (k < Lp) {
                u = fsk_u((long long)a.delay + (c0 + c - R) + (long long)k * sps, n_mf, a.mf, at);
                eu = a.e[k] * u;
            }
            t1[w] = u;
            te[w] = eu;
        }
        __syncthreads();
        trees(nc * Lp2, Lp2, true);
        if (tid < nc) {
            const float S1 = t1[tid * Lp2];
            cnum[tid] = fsk_num(Lp, te[tid * Lp2], a.se, S1);
            cs1[tid] = S1;
        }
        __syncthreads();
        for (int c = 0; c < nc; c++) {
            const float n = cnum[c];
            if (n == n && (!have || n > best)) have = true, best = n, best_S1 = cs1[c], tau = c0 + c - R;
        }
        __syncthreads();
    }
    if (!have) return fail(FSK_NO_ESTIMATE);
    const FskFit fit = fsk_fit(Lp, best, a.den, a.se, best_S1);
    if (!fsk_fit_ok(fit.dev)) return fail(FSK_NO_ESTIMATE);

    // ---- the residual of the preamble at the chosen timing
    for (int k = tid; k < Lp2; k += FSK_THREADS)
        t1[k] = k < Lp ? fsk_resid_term(fsk_u((long long)a.delay + tau + (long long)k * sps, n_mf, a.mf, at), a.e[k], fit.dev, fit.dc) : 0.0f;
    __syncthreads();
    trees(Lp2, Lp2, false);
    const float q = fsk_quality(t1[0], fit.dev, a.see);

    // ---- the data symbols, a lane each
    for (int base = 0; base < n_bits; base += FSK_THREADS) {
        const int t = base + tid;
        const bool act = t < n_bits;
        float r = 0.0f;
        if (act) {
            r = fsk_soft(fsk_u((long long)a.delay + tau + (long long)(Lp + t) * sps, n_mf, a.mf, at), fit.dc, fit.dev, a.scale);
            soft[t] = r;
        }
        if (bits) {
            const unsigned long long m = __ballot(act && r < 0.0f);
            const unsigned sub = (unsigned)(m >> (lane & ~7)) & 0xFFu;      // lane 8j's bit first
            if (act && (lane & 7) == 0) bits[t >> 3] = (uint8_t)(__brev(sub) >> 24);
        }
    }
    if (rec && tid == 0) {
        rec[0] = (float)tau, rec[1] = fit.f, rec[2] = fit.dev, rec[3] = q;
        rec[4] = rec[5] = rec[6] = rec[7] = 0.0f;
    }
    if (stat && tid == 0) *stat = FSK_OK;
}

}  // namespace

int launch_fsk_mod(const FskModArgs &a, int tx10, long long n_tiles, hipStream_t st)
{
    if (n_tiles <= 0) return SFE_OK;
    if (tx10) hipLaunchKernelGGL(fsk_mod_kernel<true>, dim3((unsigned)n_tiles), dim3(FSK_THREADS), 0, st, a);
    else hipLaunchKernelGGL(fsk_mod_kernel<false>, dim3((unsigned)n_tiles), dim3(FSK_THREADS), 0, st, a);
    SFE_HIP(hipGetLastError());
    return SFE_OK;
}

int launch_fsk_demod(const FskDemodArgs &a, int in_u8, int n_streams, hipStream_t st)
{
    const dim3 grid((unsigned)(a.n_bursts * n_streams));
    if (in_u8) hipLaunchKernelGGL(fsk_demod_kernel<true>, grid, dim3(FSK_THREADS), 0, st, a);
    else hipLaunchKernelGGL(fsk_demod_kernel<false>, grid, dim3(FSK_THREADS), 0, st, a);
    SFE_HIP(hipGetLastError());
    return SFE_OK;
}

}  // namespace sfe
