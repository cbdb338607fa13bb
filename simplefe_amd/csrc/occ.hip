// occ.hip -- the kernel of the spectrum occupancy detector (sfe_dsp_occ_*, include/sfe_dsp.h): from a row of N float32 bins to
// its floor, threshold and emission records, by the law of occ_law.h.  Compiled with -ffp-contract=off (build.py:
// EXACT_SOURCES); the host plan (api_occ.hip) compiles the same header, and the two give the same bytes.
//
// One launch, a workgroup per row: one wave at N <= 256, four waves above.  The row is read from memory once, into LDS in
// scan order, and everything after that is LDS, ballots and integer work:
//   - the floor is a selection on the 32-bit keys, which a lane keeps in registers: a bit a pass from the top, each pass a
//     count of the keys below a candidate by ballots and population counts, added over the waves through LDS (integers);
//   - occupancy, run starts, run ends and kept starts are ballots, one 64-bit word per 64 scan positions, kept in LDS;
//     what a position needs to know of the words before and behind its own -- the nearest occupied position on either
//     side, the next run end, how many kept starts and ends lie before -- is one scan of wave 0 over the (at most 64) words;
//   - closing never materialises: a run starts at an occupied position whose nearest occupied neighbour below is more than
//     `gap` away and ends at one whose neighbour above is;
//   - an emission is folded by one wave: a lane per tile of 16 positions makes the tile partials, the partials are folded
//     in ascending tile order through the wave (a read of one lane per step), the peak by a butterfly over (value, position).
// No scratch, no global or floating-point atomics, nothing that depends on which wave or workgroup finishes first.
#include "occ.h"

namespace sfe {
namespace {

constexpr int OCC_FAR = 1 << 20;            // "no such position" above every position

__device__ __forceinline__ int wave_incl_add(int v, unsigned lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(v, d);
        if (lane >= (unsigned)d) v += t;
    }
    return v;
}

__device__ __forceinline__ int wave_incl_max(int v, unsigned lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(v, d);
        if (lane >= (unsigned)d) v = max(v, t);
    }
    return v;
}

// the minimum over this lane and every lane above it
__device__ __forceinline__ int wave_suffix_min(int v, unsigned lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_down(v, d);
        if (lane + d < 64) v = min(v, t);
    }
    return v;
}

__device__ __forceinline__ unsigned long long below(int b) { return (1ull << b) - 1ull; }           // bits [0, b)
__device__ __forceinline__ unsigned long long upto(int b) { return (2ull << b) - 1ull; }            // bits [0, b]

// the first run end at or behind position p, a run start: ends[] the ends' words, nend[w] the first end in the words behind w.
// Every start has one (the last occupied position ends a run); the bound keeps an index inside the row whatever happens.
__device__ __forceinline__ int occ_run_end(const unsigned long long *ends, const int *nend, int p, int n)
{
    const unsigned long long at = ends[p >> 6] >> (p & 63);
    return min(at ? p + __builtin_ctzll(at) : nend[p >> 6], n - 1);
}

template <int T, int NMAX>
__global__ __launch_bounds__(T) void occ_kernel(OccArgs a)
{
    constexpr int NW = NMAX / 64, WAVES = T / 64, K = NMAX / T;     // a lane owns scan positions k T + tid, k < K
    __shared__ float s_x[NMAX];                                     // the row in scan order
    __shared__ unsigned s_cnt[2][WAVES];
    __shared__ unsigned long long s_occ[NW], s_start[NW], s_end[NW], s_kept[NW];    // kept: the starts of the emissions
    __shared__ unsigned s_kend[2 * NW];                             // the ends of the emissions, as 32-bit halves
    __shared__ int s_prev[NW], s_next[NW], s_nend[NW];              // per word: occupied below, occupied above, run end above
    __shared__ unsigned s_pks[NW], s_pke[NW];                       // kept starts / ends in the words before
    __shared__ unsigned s_bad[WAVES], s_count;
    __shared__ int s_lo[OCC_MAX_EMISSIONS], s_hi[OCC_MAX_EMISSIONS];

    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const int N = a.p.n, o = a.p.shift ? N >> 1 : 0, E = a.p.n_em, nw = (N + 63) >> 6;
    const unsigned s = blockIdx.x / a.n_rows, j = blockIdx.x - s * a.n_rows;
    const float *__restrict__ row = a.in + (size_t)s * (size_t)a.in_stride + (size_t)j * (size_t)N;
    const size_t q = (size_t)s * (size_t)a.out_stride + j;
    uint32_t *__restrict__ infow = reinterpret_cast<uint32_t *>(a.info + q);
    uint32_t *__restrict__ recw = reinterpret_cast<uint32_t *>(a.rec + q * (size_t)E);
    unsigned char *__restrict__ mask = a.mask ? a.mask + q * (size_t)N : nullptr;

    // ---- the row, once: into registers as keys and into LDS as values
    unsigned key[K];                    // positions past the row hold the largest key: below no candidate
    bool bad = false;
#pragma unroll
    for (int k = 0; k < K; k++) {
        const int p = k * T + (int)tid;
        key[k] = 0xffffffffu;
        if (p < N) {
            const float v = row[occ_src(p, N, o)];
            s_x[p] = v;
            bad |= !occ_finite(occ_bits(v));
            key[k] = occ_key(occ_bits(v));
        }
    }
    if (tid < 2 * NW) s_kend[tid] = 0;
    const unsigned long long anyb = __ballot(bad);
    if (lane == 0) s_bad[wave] = anyb != 0;
    __syncthreads();
    bool nonfinite = false;
#pragma unroll
    for (int w = 0; w < WAVES; w++) nonfinite |= s_bad[w] != 0;
    if (nonfinite) {                    // the whole workgroup takes this way out
        if (tid < 4) infow[tid] = tid < 2 ? OCC_QNAN : tid == 3 ? SFE_OCC_NONFINITE : 0u;
        for (int i = (int)tid; i < 8 * E; i += T) recw[i] = 0;
        if (mask)
            for (int p = (int)tid; p < N; p += T) mask[p] = 0;
        return;
    }

    // ---- the floor: the key of rank `rank` is the largest c with fewer than rank + 1 keys below it, found a bit a pass from
    // the top.  A pass counts by ballots in registers; the waves of a row add their counts through two LDS slots in turn.
    unsigned sel = 0;
    const unsigned rank = (unsigned)a.p.rank;
    for (int b = 31; b >= 0; b--) {
        const unsigned c = sel | (1u << b);
        unsigned cnt = 0;
#pragma unroll
        for (int k = 0; k < K; k++) cnt += (unsigned)__builtin_popcountll(__ballot(key[k] < c));
        if (WAVES > 1) {
            if (lane == 0) s_cnt[b & 1][wave] = cnt;
            __syncthreads();
            cnt = 0;
#pragma unroll
            for (int w = 0; w < WAVES; w++) cnt += s_cnt[b & 1][w];
        }
        if (cnt <= rank) sel = c;
    }
    const float floorv = occ_float(occ_unkey(sel));
    const float thr = occ_thr(a.p.factor, floorv, a.p.min_level);

    // ---- occupancy
#pragma unroll
    for (int k = 0; k < K; k++) {
        const unsigned long long bb = __ballot(k * T + (int)tid < N && occ_float(occ_unkey(key[k])) > thr);
        if (lane == 0) s_occ[k * WAVES + (int)wave] = bb;
    }
    __syncthreads();
    if (wave == 0) {
        const unsigned long long w = (int)lane < nw ? s_occ[lane] : 0ull;
        const int last = w ? 64 * (int)lane + 63 - __builtin_clzll(w) : -1;
        const int first = w ? 64 * (int)lane + __builtin_ctzll(w) : OCC_FAR;
        const int pm = __shfl_up(wave_incl_max(last, lane), 1), nm = __shfl_down(wave_suffix_min(first, lane), 1);
        if (lane < NW) {
            s_prev[lane] = lane ? pm : -1;
            s_next[lane] = lane < 63 ? nm : OCC_FAR;
        }
    }
    __syncthreads();

    // ---- the runs of the closing: where they start and end
    for (int base = 0; base < N; base += T) {
        const int p = base + (int)tid;
        bool st = false, en = false;
        if (p < N) {
            const int w = p >> 6, b = p & 63;
            const unsigned long long word = s_occ[w];
            if ((word >> b) & 1ull) {
                const unsigned long long lo = word & below(b), hi = (word >> b) >> 1;
                const int pa = lo ? 64 * w + 63 - __builtin_clzll(lo) : s_prev[w];
                const int pb = hi ? p + 1 + __builtin_ctzll(hi) : s_next[w];
                st = pa < 0 || p - pa - 1 > a.p.gap;
                en = pb >= OCC_FAR || pb - p - 1 > a.p.gap;
            }
        }
        const unsigned long long bs = __ballot(st), be = __ballot(en);
        if (lane == 0) {
            s_start[(base >> 6) + wave] = bs;
            s_end[(base >> 6) + wave] = be;
        }
    }
    __syncthreads();
    if (wave == 0) {
        const unsigned long long w = (int)lane < nw ? s_end[lane] : 0ull;
        const int first = w ? 64 * (int)lane + __builtin_ctzll(w) : OCC_FAR;
        const int nm = __shfl_down(wave_suffix_min(first, lane), 1);
        if (lane < NW) s_nend[lane] = lane < 63 ? nm : OCC_FAR;
    }
    __syncthreads();

    // ---- the runs wide enough are the emissions
    for (int base = 0; base < N; base += T) {
        const int p = base + (int)tid;
        bool keep = false;
        if (p < N && ((s_start[p >> 6] >> (p & 63)) & 1ull)) {
            const int hi = occ_run_end(s_end, s_nend, p, N);
            keep = hi - p + 1 >= a.p.min_width;
            if (keep) atomicOr(&s_kend[hi >> 5], 1u << (hi & 31));
        }
        const unsigned long long bk = __ballot(keep);
        if (lane == 0) s_kept[(base >> 6) + wave] = bk;
    }
    __syncthreads();
    if (wave == 0) {
        const bool in = (int)lane < nw;
        const unsigned long long ks = in ? s_kept[lane] : 0ull;
        const unsigned long long ke = in ? ((unsigned long long)s_kend[2 * lane + 1] << 32) | s_kend[2 * lane] : 0ull;
        const int cs = __builtin_popcountll(ks), ce = __builtin_popcountll(ke);
        const int is = wave_incl_add(cs, lane), ie = wave_incl_add(ce, lane);
        if (lane < NW) {
            s_pks[lane] = (unsigned)(is - cs);
            s_pke[lane] = (unsigned)(ie - ce);
        }
        if (lane == 63) s_count = (unsigned)is;
    }
    __syncthreads();

    // ---- the mask, the emissions' bounds, info, and the records nobody fills
    const unsigned count = s_count, ne = min(count, (unsigned)E);
    for (int base = 0; base < N; base += T) {
        const int p = base + (int)tid;
        if (p < N) {
            const int w = p >> 6, b = p & 63;
            const unsigned long long ks = s_kept[w], ke = ((unsigned long long)s_kend[2 * w + 1] << 32) | s_kend[2 * w];
            const unsigned ns = s_pks[w] + (unsigned)__builtin_popcountll(ks & upto(b));
            const unsigned nend = s_pke[w] + (unsigned)__builtin_popcountll(ke & below(b));
            if (mask) mask[occ_src(p, N, o)] = (unsigned char)(ns - nend);         // 1 inside an emission, 0 outside
            if (((ks >> b) & 1ull) && ns - 1 < (unsigned)E) {
                s_lo[ns - 1] = p;
                s_hi[ns - 1] = occ_run_end(s_end, s_nend, p, N);
            }
        }
    }
    if (tid == 0) {
        infow[0] = occ_bits(floorv);
        infow[1] = occ_bits(thr);
        infow[2] = count;
        infow[3] = count > (unsigned)E ? SFE_OCC_TRUNCATED : 0u;
    }
    for (int i = 8 * (int)ne + (int)tid; i < 8 * E; i += T) recw[i] = 0;
    __syncthreads();

    // ---- an emission per wave at a time
    for (unsigned e = wave; e < ne; e += WAVES) {
        const int lo = __builtin_amdgcn_readfirstlane(s_lo[e]), hi = __builtin_amdgcn_readfirstlane(s_hi[e]);
        const int t0 = lo >> OCC_TILE_LOG2, t1 = hi >> OCC_TILE_LOG2;
        float sum = 0.0f, mom = 0.0f, bv = -INFINITY;
        int bp = 0x7fffffff;
        for (int c0 = t0; c0 <= t1; c0 += 64) {
            const int t = c0 + (int)lane;
            float ps = 0.0f, pm = 0.0f;
            if (t <= t1) {
                const int pa = max(lo, t << OCC_TILE_LOG2), pb = min(hi, (t << OCC_TILE_LOG2) + (1 << OCC_TILE_LOG2) - 1);
                for (int p = pa; p <= pb; p++) {
                    const float x = s_x[p];
                    ps = occ_sum_step(ps, x);
                    pm = occ_mom_step(pm, p - lo, x);
                    if (occ_better(x, p, bv, bp)) {
                        bv = x;
                        bp = p;
                    }
                }
            }
            const int nt = min(64, t1 - c0 + 1);
            for (int i = 0; i < nt; i++) {              // the tile partials in ascending t, the same chain in every lane
                sum = occ_sum_step(sum, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ps), i)));
                mom = occ_sum_step(mom, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(pm), i)));
            }
        }
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const float ov = __shfl_xor(bv, d);
            const int op = __shfl_xor(bp, d);
            if (occ_better(ov, op, bv, bp)) {
                bv = ov;
                bp = op;
            }
        }
        if (lane < 8) {
            const uint32_t f = lane == 0 ? (uint32_t)(lo - o) : lane == 1 ? (uint32_t)(hi - o) : lane == 2 ? (uint32_t)(bp - o)
                             : lane == 3 ? occ_bits(bv) : lane == 4 ? occ_bits(sum) : lane == 5 ? occ_bits(mom) : 0u;
            recw[8 * e + lane] = f;
        }
    }
}

}  // namespace

int launch_occ(const OccArgs &a, unsigned n_streams, hipStream_t st)
{
    const unsigned rows = n_streams * a.n_rows;
    if (a.p.n <= 256) hipLaunchKernelGGL((occ_kernel<64, 256>), dim3(rows), dim3(64), 0, st, a);
    else if (a.p.n <= 1024) hipLaunchKernelGGL((occ_kernel<256, 1024>), dim3(rows), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((occ_kernel<256, OCC_MAX_BINS>), dim3(rows), dim3(256), 0, st, a);
    SFE_HIP(hipGetLastError());
    return SFE_OK;
}

}  // namespace sfe
