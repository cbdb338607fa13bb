// ddc.hip -- digital down-converter bank (sfe_dsp_ddc_*): K tunings of a stream, each shifted to baseband, low-pass
// filtered by one real prototype and decimated by D, from one pass over the input.
//
//   y_k[m] = sum_{n<L} h[n] x[mD - n] exp(-j 2 pi phi_k(mD - n) / 2^32),   phi_k(i) = (i inc_k) mod 2^32
//          = exp(-j 2 pi phi_k(mD) / 2^32) sum_{r<D} sum_{j<P} g_k[r + jD] u_r[m - j],
//   g_k[n] = h[n] exp(+j 2 pi phi_k(n) / 2^32)  (the host's table, made in float64),   u_r[b] = x[bD - r]
// (the phase is linear mod 2^32, so the taps are rotated instead of the data).
//
// One workgroup (256 threads) owns G T consecutive output instants of one stream and one chunk of KT tunings (the grid
// holds every chunk of every tile), G = 256 / min(D, 256) sub-tiles of T instants, one per group of min(D, 256) lanes:
//   1. branch sums.  Lane e of a group owns branches r = e, e + 256, ... (D > 256: in turn, into the same sums).  Its
//      T x KT complex accumulators stay in registers; the taps go through in chunks of DDC_RU rows, each chunk loading
//      the window of T + DDC_RU - 1 branch samples u_r[b] it needs (contiguous across lanes) and making DDC_RU x KT x T
//      complex multiply-adds with static register indices.  Every output sums its terms in the same order (branch pass,
//      tap row) wherever the call or the tile starts.
//   2. the D branch sums of each (instant, tuning) are added in LDS in a fixed order: segments of lanes in ascending e,
//      then the segments in ascending order.  The split depends on D and T only, so cutting a stream at any multiple of
//      D gives the one-call bits.
//   3. the lead factor exp(-j 2 pi phi_k(mD) / 2^32), from the absolute sample index (the host's counter mod 2^32 plus
//      m D) by ocml sincospi on the signed phase, and channel-major stores: tuning k of stream s at
//      out + (s K + k) out_stride + m, lanes along m.
// The carried history (H = P D samples per stream, cf32 for complex input whatever its format, float for real input;
// zero at create / reset) is read for x[i < 0]; ddc_hist_kernel writes the next call's into the other buffer of the pair.
#include <algorithm>
#include <type_traits>

#include "common.h"

namespace sfe {

namespace {

constexpr int DDC_THREADS = 256;
constexpr int DDC_RU = 4;       // tap rows per chunk; the host pads P to a multiple of it with zero taps
constexpr int DDC_RED = 16;     // (instant, tuning) slots per lane in one LDS reduction round

enum { DDC_CF32 = 0, DDC_U8 = 1, DDC_REAL = 2 };

// instants per sub-tile for KT tunings per chunk (T x KT accumulators of 2 floats: 32 to 128 registers), and the waves per
// SIMD the register budget is set for
constexpr int ddc_instants(int kt) { return kt >= 4 ? 8 : 16; }
constexpr int ddc_waves(int kt) { return kt == 8 ? 2 : kt == 2 ? 3 : 4; }

struct DdcArgs {
    const void *in;             // call input: stream s at in + s in_stride samples (cf32, u8 (I,Q) pairs or real float)
    const void *hist;           // [n_streams][H]: the H samples before the call, oldest first (cf32, or float for real)
    void *hist_next;            // [n_streams][H]: written by ddc_hist_kernel
    const v2f *taps;            // [Kpad / KT][P][D][KT] = g_k zero-padded, chunks of KT tunings
    const unsigned *inc;        // [Kpad] phase increments (zero past K)
    v2f *out;
    long long in_stride, out_stride;
    int n_in, n_out, D, P, H, K, Kpad, n_streams;   // P a multiple of DDC_RU, Kpad of the kernel's KT; n_in < 2^31
    int tiles, t_lo, t_hi;      // tiles per stream; [t_lo, t_hi) are interior: every sample they read is one of the call
                                // and every instant an output of it
    unsigned c0;                // absolute index of the call's first input sample, mod 2^32
};

template <int FMT>
using ddc_sample_t = typename std::conditional<FMT == DDC_REAL, float, v2f>::type;     // a sample after loading
template <int FMT>
using ddc_wire_t = typename std::conditional<FMT == DDC_U8, unsigned short, ddc_sample_t<FMT>>::type;   // as stored

template <int FMT>
__device__ __forceinline__ ddc_sample_t<FMT> ddc_load(const ddc_wire_t<FMT> *p)
{
    if constexpr (FMT == DDC_U8) {
        const unsigned w = *p;
        return v2f{u8_to_f32(w & 0xffu), u8_to_f32(w >> 8)};
    } else {
        return *p;
    }
}

// acc += g x, g complex; x complex (two packed multiply-adds, the second on xs = j x = {-x.y, x.x}, made once per window
// slot, so that the taps need no negated copy) or real (one)
__device__ __forceinline__ v2f ddc_mac(v2f g, v2f x, v2f xs, v2f acc)
{
    acc = __builtin_elementwise_fma(v2f{g.x, g.x}, x, acc);
    return __builtin_elementwise_fma(v2f{g.y, g.y}, xs, acc);
}
__device__ __forceinline__ v2f ddc_mac(v2f g, float x, float, v2f acc) { return __builtin_elementwise_fma(g, v2f{x, x}, acc); }
__device__ __forceinline__ v2f ddc_rot(v2f x) { return v2f{-x.y, x.x}; }
__device__ __forceinline__ float ddc_rot(float x) { return x; }

// step 1 for branch r of sub-tile g, chunk kci of KT tunings: acc[t][k] += sum_j g_k[r + jD] u_r[mt + t - j], mt = mtile + gT.
// Sample (mtile + c) D - r is row base (mtile + c) D - (D - 1) (uniform) plus lane offset lo = g T D + D - 1 - r >= 0, and
// the KT taps of row j are contiguous at a uniform row base plus r KT: the loads take one address register each.  D is
// re-read each chunk through an opaque copy, so that the W row offsets q D are not hoisted into W scalar register pairs.
template <int FMT, int KT, int T, bool GUARD>
__device__ __forceinline__ void ddc_branch(const DdcArgs &a, const ddc_wire_t<FMT> *in, const ddc_sample_t<FMT> *hist, int mtile,
                                           int mt, int lo, int r, int kci, v2f (&acc)[T][KT])
{
    using X = ddc_sample_t<FMT>;
    constexpr int W = T + DDC_RU - 1;
#pragma unroll 1
    for (int r0 = 0; r0 < a.P; r0 += DDC_RU) {
        int D = a.D;
        asm volatile("" : "+s"(D));
        X w[W];
#pragma unroll
        for (int q = 0; q < W; q++) {
            const int c = q - (r0 + DDC_RU - 1), ib = (mtile + c) * D - (D - 1);
            if constexpr (GUARD) {
                const int b = mt + c, i = ib + lo;
                if (b >= a.n_out) w[q] = X{};                               // past the last output of the call: never used
                else if (i < 0) w[q] = hist[a.H + i];
                else w[q] = ddc_load<FMT>(in + ib + lo);
            } else {
                w[q] = ddc_load<FMT>(in + ib + lo);
            }
        }
        X ws[W];
#pragma unroll
        for (int q = 0; q < W; q++) ws[q] = ddc_rot(w[q]);
        // tap row ii + 1 is loaded while row ii is used; the scheduling barrier keeps the compiler from loading every row of
        // the chunk at once (4 KT more registers)
        auto taps_of = [&](int ii, v2f (&gk)[KT]) {
            const v2f *row = a.taps + ((kci * a.P + r0 + ii) * D) * KT;      // the table holds fewer than 2^22 taps
#pragma unroll
            for (int k = 0; k < KT; k++) gk[k] = row[r * KT + k];
        };
        v2f gk[2][KT];
        taps_of(0, gk[0]);
#pragma unroll
        for (int ii = 0; ii < DDC_RU; ii++) {
            if (ii + 1 < DDC_RU) taps_of(ii + 1, gk[(ii + 1) & 1]);
#pragma unroll
            for (int k = 0; k < KT; k++)
#pragma unroll
                for (int t = 0; t < T; t++) acc[t][k] = ddc_mac(gk[ii & 1][k], w[t - ii + DDC_RU - 1], ws[t - ii + DDC_RU - 1], acc[t][k]);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

// GUARD: the launch over the edge tiles (history, the call's end), with every load checked; its own kernel, so that the
// checks do not cost the interior kernel registers
template <int FMT, int KT, int T, bool GUARD>
__global__ __launch_bounds__(DDC_THREADS, GUARD ? 1 : ddc_waves(KT)) void ddc_kernel(DdcArgs a)
{
    constexpr int KR = DDC_RED / T;                         // tunings per reduction round
    static_assert(KR >= 1 && KT % KR == 0, "whole reduction rounds");
    // [KR][T][G E]: one round's branch sums, rows padded by one sample so that the readers of step 2, one (instant, tuning)
    // each, hit different banks
    __shared__ v2f S[(DDC_THREADS + 1) * DDC_RED];
    __shared__ v2f Q[DDC_THREADS];                          // [segment][output]: partial sums

    // block b runs work item u = 8 (b / 8 NKC) + b % 8 for tunings kc .. kc + KT - 1, kc = KT ((b / 8) mod NKC): the NKC
    // chunks of a tile go to the same XCD (blocks are dealt to the 8 XCDs in turn) and read its input from one L2
    const int NKC = a.Kpad / KT, b = blockIdx.x;
    const int u = (b / (8 * NKC)) * 8 + b % 8, kc = (b / 8) % NKC * KT;
    const int ni = a.t_hi - a.t_lo, nt = GUARD ? a.tiles - ni : ni;
    if (u >= nt * a.n_streams) return;
    const int s = u / nt, j = u % nt;
    const int tile = GUARD ? (j < a.t_lo ? j : a.t_hi + j - a.t_lo) : a.t_lo + j;
    const int tid = threadIdx.x;
    const int E = a.D < DDC_THREADS ? a.D : DDC_THREADS, G = DDC_THREADS / E, NL = G * E;
    const int GT = G * T, mtile = tile * GT;
    const int g = tid / E, e = tid - g * E, mt = mtile + g * T;
    const auto *in = static_cast<const ddc_wire_t<FMT> *>(a.in) + s * a.in_stride;
    const auto *hist = static_cast<const ddc_sample_t<FMT> *>(a.hist) + (long long)s * a.H;
    v2f *out = a.out + (long long)s * a.K * a.out_stride;

    // the split of step 2: nseg segments of seg lanes per (instant, tuning) sum, from D and T only
    const int O = KR * GT;
    int nseg = O >= DDC_THREADS ? 1 : min(E, DDC_THREADS / O);
    const int seg = (E + nseg - 1) / nseg;
    nseg = (E + seg - 1) / seg;

    v2f acc[T][KT];
#pragma unroll
    for (int t = 0; t < T; t++)
#pragma unroll
        for (int k = 0; k < KT; k++) acc[t][k] = v2f{0.0f, 0.0f};
    if (tid < NL) {
#pragma unroll 1
        for (int r = e; r < a.D; r += DDC_THREADS) {
            const int lo = g * T * a.D + a.D - 1 - r;
            ddc_branch<FMT, KT, T, GUARD>(a, in, hist, mtile, mt, lo, r, kc / KT, acc);
        }
    }
    // step 2 computes its LDS addresses from copies of tid and NL the compiler cannot see through: hoisted above step 1,
    // the KT T store addresses alone would hold as many registers there
    int ftid = tid, fNL = NL;
    asm volatile("" : "+v"(ftid), "+s"(fNL));
#pragma unroll
    for (int k1 = 0; k1 < KT; k1 += KR) {
        lds_barrier();                                  // the previous round's readers are done with S
        if (ftid < fNL) {
#pragma unroll
            for (int k = 0; k < KR; k++)
#pragma unroll
                for (int t = 0; t < T; t++) S[(k * T + t) * (fNL + 1) + ftid] = acc[t][k1 + k];
        }
        lds_barrier();
        // output o = (k G + g') T + t' of the round: instant mtile + g' T + t', tuning kc + k1 + k
        auto finish = [&](int o, v2f v) {
            const int k = kc + k1 + o / GT, m = mtile + o % GT;
            if (m >= a.n_out || k >= a.K) return;
            const unsigned ph = (a.c0 + (unsigned)m * (unsigned)a.D) * a.inc[k];
            float sn, cs;
            sincospif((float)(int)ph * 0x1p-31f, &sn, &cs);          // the signed phase, in half turns
            out[k * a.out_stride + m] = v2f{fmaf(v.x, cs, v.y * sn), fmaf(v.y, cs, -(v.x * sn))};
        };
        auto base = [&](int o) { return ((o / GT) * T + o % T) * (NL + 1) + ((o % GT) / T) * E; };
        if (nseg == 1) {
            for (int o = tid; o < O; o += DDC_THREADS) {
                const v2f *p = S + base(o);
                v2f v = v2f{0.0f, 0.0f};
                for (int i = 0; i < E; i++) v += p[i];
                finish(o, v);
            }
        } else {
            if (tid < O * nseg) {
                const int o = tid % O, sg = tid / O, i1 = min(E, (sg + 1) * seg);
                const v2f *p = S + base(o);
                v2f v = v2f{0.0f, 0.0f};
                for (int i = sg * seg; i < i1; i++) v += p[i];
                Q[sg * O + o] = v;
            }
            lds_barrier();
            if (tid < O) {
                v2f v = v2f{0.0f, 0.0f};
                for (int sg = 0; sg < nseg; sg++) v += Q[sg * O + tid];
                finish(tid, v);
            }
        }
    }
}

// the H samples that end the call (old history followed by the call's input) into hist_next, as cf32 (or float)
template <int FMT>
__global__ __launch_bounds__(256) void ddc_hist_kernel(DdcArgs a)
{
    using X = ddc_sample_t<FMT>;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int s = blockIdx.y;
    if (i >= a.H) return;
    const int src = a.n_in - a.H + i;
    const auto *in = static_cast<const ddc_wire_t<FMT> *>(a.in) + s * a.in_stride;
    const X *hist = static_cast<const X *>(a.hist) + (long long)s * a.H;
    static_cast<X *>(a.hist_next)[(long long)s * a.H + i] = src >= 0 ? ddc_load<FMT>(in + src) : hist[a.H + src];
}

template <int FMT, int KT>
void ddc_launch_one(const DdcArgs &a, hipStream_t st)
{
    constexpr int T = ddc_instants(KT);
    const int ni = a.t_hi - a.t_lo, NKC = a.Kpad / KT;
    if (ni > 0)
        hipLaunchKernelGGL((ddc_kernel<FMT, KT, T, false>), dim3((ni * a.n_streams + 7) / 8 * 8 * NKC), dim3(DDC_THREADS), 0, st, a);
    if (a.tiles > ni)
        hipLaunchKernelGGL((ddc_kernel<FMT, KT, T, true>), dim3(((a.tiles - ni) * a.n_streams + 7) / 8 * 8 * NKC), dim3(DDC_THREADS),
                           0, st, a);
}

template <int FMT>
void ddc_launch_fmt(const DdcArgs &a, int kt, hipStream_t st)
{
    switch (kt) {
    case 1: ddc_launch_one<FMT, 1>(a, st); break;
    case 2: ddc_launch_one<FMT, 2>(a, st); break;
    case 4: ddc_launch_one<FMT, 4>(a, st); break;
    default: ddc_launch_one<FMT, 8>(a, st); break;
    }
    if (a.n_in > 0) {
        const dim3 grid((unsigned)((a.H + 255) / 256), (unsigned)a.n_streams);
        hipLaunchKernelGGL(ddc_hist_kernel<FMT>, grid, dim3(256), 0, st, a);
    }
}

}  // namespace

// tunings per chunk of the kernel for K tunings (the host pads the tap table to a multiple of it)
int ddc_tunings_per_chunk(int K) { return K == 1 ? 1 : K == 2 ? 2 : K <= 4 ? 4 : 8; }

// One call: the down-converter bank over n_in samples of every stream, then the history update.  Shapes and buffers are
// the caller's (api_ddc.hip) to check: 1 <= D <= 1024, P a multiple of DDC_RU, H = P D, Kpad a multiple of
// ddc_tunings_per_chunk(K), n_in a multiple of D below 2^31.  fmt: 0 cf32, 1 u8 (I,Q), 2 real float.
int launch_ddc(int fmt, const void *in, long long in_stride, const void *hist, void *hist_next, const v2f *taps,
               const unsigned *inc, v2f *out, long long out_stride, long long n_in, int D, int P, int H, int K, int Kpad,
               unsigned c0, int n_streams, hipStream_t st)
{
    const int n_out = (int)(n_in / D), kt = ddc_tunings_per_chunk(K);
    const int rows = (DDC_THREADS / (D < DDC_THREADS ? D : DDC_THREADS)) * ddc_instants(kt);
    const long long tiles = ((long long)n_out + rows - 1) / rows;
    if ((tiles * n_streams + 7) / 8 * 8 * (Kpad / kt) > 0x7fffffffLL || n_streams > 65535) {
        set_error("ddc_process_stream: call too large for one grid");
        return SFE_EINVAL;
    }
    if (n_in <= 0) return SFE_OK;
    // a tile is interior from its first instant m >= P - 1 (+1 for D > 1: sample mD - (P - 1) D - (D - 1) >= 0) until it
    // would pass the call's last output
    const int m_lo = P - 1 + (D > 1), t_lo = (int)std::min<long long>(tiles, (m_lo + rows - 1) / rows);
    const int t_hi = std::max(t_lo, n_out / rows);
    DdcArgs a{in, hist, hist_next, taps, inc, out, in_stride, out_stride, (int)n_in, n_out, D, P, H, K, Kpad, n_streams,
              (int)tiles, t_lo, t_hi, c0};
    if (fmt == DDC_U8) ddc_launch_fmt<DDC_U8>(a, kt, st);
    else if (fmt == DDC_REAL) ddc_launch_fmt<DDC_REAL>(a, kt, st);
    else ddc_launch_fmt<DDC_CF32>(a, kt, st);
    SFE_HIP(hipGetLastError());
    return SFE_OK;
}

}  // namespace sfe
