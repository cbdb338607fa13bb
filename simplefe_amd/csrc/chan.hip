// chan.hip -- polyphase filter-bank channelizer (sfe_dsp_chan_*): M sub-bands of a complex stream in one pass.
//
//   y_k[m] = sum_{n<L} h[n] x[mD - n] exp(-j 2 pi k (mD - n) / M),   D = M or M/2
//          = exp(-j 2 pi k mD / M) sum_p W^{kp} v_p[m],  W = exp(+j 2 pi / M),  v_p[m] = sum_r h[p + rM] x[mD - p - rM]
//
// One workgroup (256 threads) owns ROWS consecutive output instants of one stream:
//   1. branch sums.  Thread owns branch p (and M/256 of them in turn for M > 256; for M < 256 the workgroup holds 256/M
//      sub-tiles of T instants, one per group of M lanes).  Its T accumulators stay in registers; the taps go through in
//      chunks of RU rows, each chunk loading the window of T + SH(RU-1) branch samples u_p[b] = x[bD - p] it needs (loads
//      contiguous across lanes) and making RU x T multiply-adds with static register indices.  The P-1 rows before the
//      sub-tile are re-read (from cache).  Every output sums its taps in the same order, r = 0, 1, ..., P-1, wherever
//      the call or the tile starts: cutting a stream at any multiple of D gives the same bits.
//   2. the sums go to LDS, one padded row of M per instant.  For D = M/2 the leading factor is (-1)^(km): on odd
//      absolute m the row is written rotated by M/2 (an index permutation, no multiply).
//   3. an unnormalised inverse M-point DFT per row in LDS: self-sorting (Stockham) radix-4 passes, one radix-2 pass
//      first when log2 M is odd, twiddles from a table of exp(+j 2 pi q / M).
//   4. channel k of each instant goes out to out + (s M + k) out_stride + m: lanes run along m, so a channel's
//      ROWS instants are one contiguous run.
// The carried history (H = P M samples per stream, cf32, zero at create/reset) is read for x[i < 0]; chan_hist_kernel
// writes the next call's history into the other buffer of the pair behind the main launch.
#include "fft16.h"

namespace sfe {

namespace {

constexpr int CHAN_THREADS = 256;
constexpr int CHAN_RU = 8;      // tap rows per chunk; the host pads P to a multiple of it with zero taps

struct ChanArgs {
    const void *in;             // call input: stream s at in + s in_stride samples (cf32, or u8 (I,Q) pairs)
    const v2f *hist;            // [n_streams][H]: the H samples before the call, oldest first
    v2f *hist_next;             // [n_streams][H]: written by chan_hist_kernel
    const float *taps;          // [P][M] = h zero-padded to P M
    const v2f *tw;              // [M]: exp(+j 2 pi q / M)
    v2f *out;
    long long in_stride, out_stride, n_in, n_out;
    int P, H, parity, tiles;    // P a multiple of CHAN_RU; parity: absolute index of the call's first output, mod 2
};

template <bool U8>
__device__ __forceinline__ v2f chan_load(const void *base, long long i)
{
    if constexpr (U8) {
        const unsigned w = static_cast<const unsigned short *>(base)[i];
        return v2f{u8_to_f32(w & 0xffu), u8_to_f32(w >> 8)};
    } else {
        return static_cast<const v2f *>(base)[i];
    }
}

__device__ __forceinline__ v2f chan_fma(float h, v2f x, v2f acc) { return __builtin_elementwise_fma(v2f{h, h}, x, acc); }

// step 1 for one branch p: acc[j] = v_p[mt + j]
template <int LOGM, bool HALF, bool U8, bool GUARD, int T>
__device__ __forceinline__ void chan_branch(const ChanArgs &a, const void *in, const v2f *hist, long long mt, int p, v2f (&acc)[T])
{
    constexpr int M = 1 << LOGM, D = HALF ? M / 2 : M, SH = HALF ? 2 : 1, W = T + SH * (CHAN_RU - 1);
    for (int j = 0; j < T; j++) acc[j] = v2f{0.0f, 0.0f};
    for (int r0 = 0; r0 < a.P; r0 += CHAN_RU) {
        float h[CHAN_RU];
#pragma unroll
        for (int i = 0; i < CHAN_RU; i++) h[i] = a.taps[(r0 + i) * M + p];
        const long long b0 = mt - SH * (r0 + CHAN_RU - 1);
        v2f w[W];
#pragma unroll
        for (int q = 0; q < W; q++) {
            const long long b = b0 + q, i = b * D - p;
            if constexpr (GUARD) {
                if (b >= a.n_out) w[q] = v2f{0.0f, 0.0f};          // past the last output of the call: never used
                else if (i < 0) w[q] = hist[a.H + i];
                else w[q] = chan_load<U8>(in, i);
            } else {
                w[q] = chan_load<U8>(in, i);
            }
        }
        // acc[j] += h[r0 + i] u_p[mt + j - SH (r0 + i)]
#pragma unroll
        for (int i = 0; i < CHAN_RU; i++)
#pragma unroll
            for (int j = 0; j < T; j++) acc[j] = chan_fma(h[i], w[j - SH * i + SH * (CHAN_RU - 1)], acc[j]);
    }
}

// one Stockham pass of radix R over ROWS rows of M in LDS: sub-transforms of length Ls = 2^logLs become R Ls long
template <int LOGM, int ROWS, int RS, int R>
__device__ __forceinline__ void chan_pass(v2f *V, const v2f *tw, int logLs, int tid)
{
    constexpr int M = 1 << LOGM, NQ = M / R, NI = ROWS * NQ / CHAN_THREADS, LOGR = R == 4 ? 2 : 1;
    static_assert(NI * CHAN_THREADS == ROWS * NQ, "whole passes per thread");
    const int Ls = 1 << logLs;
    v2f y[NI][R];
#pragma unroll
    for (int e = 0; e < NI; e++) {
        const int it = e * CHAN_THREADS + tid, row = it / NQ, j = it % NQ, k = j & (Ls - 1);
        v2f x[R];
#pragma unroll
        for (int r = 0; r < R; r++) x[r] = V[row * RS + j + r * NQ];
        if (logLs > 0) {
#pragma unroll
            for (int r = 1; r < R; r++) x[r] = cmul(x[r], tw[(r * k) << (LOGM - logLs - LOGR)]);
        }
        if constexpr (R == 4) {
            const v2f t0 = x[0] + x[2], t1 = x[0] - x[2], t2 = x[1] + x[3], t3 = x[1] - x[3];
            y[e][0] = t0 + t2;
            y[e][1] = add_pj(t1, t3);       // x0 + j x1 - x2 - j x3
            y[e][2] = t0 - t2;
            y[e][3] = add_mj(t1, t3);
        } else {
            y[e][0] = x[0] + x[1];
            y[e][1] = x[0] - x[1];
        }
    }
    lds_barrier();
#pragma unroll
    for (int e = 0; e < NI; e++) {
        const int it = e * CHAN_THREADS + tid, row = it / NQ, j = it % NQ, k = j & (Ls - 1);
        const int base = ((j >> logLs) << (logLs + LOGR)) + k;
#pragma unroll
        for (int r = 0; r < R; r++) V[row * RS + base + r * Ls] = y[e][r];
    }
    lds_barrier();
}

template <int LOGM, bool HALF, bool U8>
__global__ __launch_bounds__(CHAN_THREADS) void chan_kernel(ChanArgs a)
{
    constexpr int M = 1 << LOGM, D = HALF ? M / 2 : M, SH = HALF ? 2 : 1;
    constexpr int T = M <= 256 ? 16 : 8;                    // instants per sub-tile
    constexpr int G = M < 256 ? 256 / M : 1;                // sub-tiles per workgroup
    constexpr int NB = M > 256 ? M / 256 : 1;               // branches per thread, in turn
    constexpr int ROWS = G * T, RS = M + 1;                 // row stride M + 1: the column reads of step 4 are conflict-free
    __shared__ v2f V[ROWS * RS];

    const int tid = threadIdx.x;
    const int s = blockIdx.x / a.tiles, tile = blockIdx.x % a.tiles;
    const long long mtile = (long long)tile * ROWS;
    const void *in = static_cast<const char *>(a.in) + s * a.in_stride * (U8 ? 2 : 8);
    const v2f *hist = a.hist + (long long)s * a.H;
    const int g = M < 256 ? tid >> LOGM : 0;
    const long long mt = mtile + g * T;
    // every row the workgroup reads is a sample of this call, and every instant is an output of it
    const bool interior = (mtile - (long long)SH * (a.P - 1)) * D - (M - 1) >= 0 && mtile + ROWS <= a.n_out;

#pragma unroll
    for (int q = 0; q < NB; q++) {
        const int p = M < 256 ? (tid & (M - 1)) : tid + CHAN_THREADS * q;
        v2f acc[T];
        if (interior) chan_branch<LOGM, HALF, U8, false, T>(a, in, hist, mt, p, acc);
        else chan_branch<LOGM, HALF, U8, true, T>(a, in, hist, mt, p, acc);
#pragma unroll
        for (int j = 0; j < T; j++) {
            const bool odd = HALF && ((a.parity + mt + j) & 1);
            V[(g * T + j) * RS + (odd ? (p + M / 2) & (M - 1) : p)] = acc[j];
        }
    }
    lds_barrier();

    int logLs = 0;
    if constexpr (LOGM & 1) {
        chan_pass<LOGM, ROWS, RS, 2>(V, a.tw, 0, tid);
        logLs = 1;
    }
#pragma unroll
    for (; logLs < LOGM; logLs += 2) chan_pass<LOGM, ROWS, RS, 4>(V, a.tw, logLs, tid);

    constexpr int NO = ROWS * M / CHAN_THREADS;
    v2f *out = a.out + (long long)s * M * a.out_stride;
#pragma unroll
    for (int e = 0; e < NO; e++) {
        const int it = e * CHAN_THREADS + tid, k = it / ROWS, jm = it % ROWS;
        const long long m = mtile + jm;
        if (m < a.n_out) out[k * a.out_stride + m] = V[jm * RS + k];
    }
}

// the H samples that end the call (old history followed by the call's input), as cf32, into hist_next
template <bool U8>
__global__ __launch_bounds__(256) void chan_hist_kernel(ChanArgs a)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int s = blockIdx.y;
    if (i >= a.H) return;
    const long long src = a.n_in - a.H + i;
    const void *in = static_cast<const char *>(a.in) + s * a.in_stride * (U8 ? 2 : 8);
    a.hist_next[(long long)s * a.H + i] = src >= 0 ? chan_load<U8>(in, src) : a.hist[(long long)s * a.H + a.H + src];
}

template <int LOGM, bool HALF, bool U8>
int chan_launch_one(const ChanArgs &a, int n_streams, hipStream_t st)
{
    hipLaunchKernelGGL((chan_kernel<LOGM, HALF, U8>), dim3(a.tiles * n_streams), dim3(CHAN_THREADS), 0, st, a);
    SFE_HIP(hipGetLastError());
    return SFE_OK;
}

template <int LOGM>
int chan_launch_m(const ChanArgs &a, int half, int u8, int n_streams, hipStream_t st)
{
    if (half) return u8 ? chan_launch_one<LOGM, true, true>(a, n_streams, st) : chan_launch_one<LOGM, true, false>(a, n_streams, st);
    return u8 ? chan_launch_one<LOGM, false, true>(a, n_streams, st) : chan_launch_one<LOGM, false, false>(a, n_streams, st);
}

}  // namespace

// instants per workgroup of the kernel for 2^logm channels (the host sizes the grid with it)
int chan_tile_rows(int logm) { return logm <= 8 ? 16 * (256 >> logm) : 8; }

// One call: the channelizer over n_in samples of every stream, then the history update.  Shapes and buffers are the
// caller's (api_chan.hip) to check: 2 <= logm <= 10, P a multiple of CHAN_RU, H = P M, n_in a multiple of D.
int launch_chan(int logm, int half, int u8, const void *in, long long in_stride, const v2f *hist, v2f *hist_next,
                const float *taps, const v2f *tw, v2f *out, long long out_stride, long long n_in, long long n_out, int P, int H,
                int parity, int n_streams, hipStream_t st)
{
    ChanArgs a{in, hist, hist_next, taps, tw, out, in_stride, out_stride, n_in, n_out, P, H, parity, 0};
    const long long rows = chan_tile_rows(logm);
    const long long tiles = (n_out + rows - 1) / rows;
    if (tiles * n_streams > 0x7fffffffLL || (H + 255LL) / 256 > 0x7fffffffLL) {
        set_error("chan_process_stream: call too large for one grid");
        return SFE_EINVAL;
    }
    a.tiles = (int)tiles;
    int rc = SFE_OK;
    if (n_out > 0) {
        switch (logm) {
        case 2: rc = chan_launch_m<2>(a, half, u8, n_streams, st); break;
        case 3: rc = chan_launch_m<3>(a, half, u8, n_streams, st); break;
        case 4: rc = chan_launch_m<4>(a, half, u8, n_streams, st); break;
        case 5: rc = chan_launch_m<5>(a, half, u8, n_streams, st); break;
        case 6: rc = chan_launch_m<6>(a, half, u8, n_streams, st); break;
        case 7: rc = chan_launch_m<7>(a, half, u8, n_streams, st); break;
        case 8: rc = chan_launch_m<8>(a, half, u8, n_streams, st); break;
        case 9: rc = chan_launch_m<9>(a, half, u8, n_streams, st); break;
        case 10: rc = chan_launch_m<10>(a, half, u8, n_streams, st); break;
        default: set_error("chan: log2 M = %d has no kernel", logm); return SFE_EINVAL;
        }
        if (rc != SFE_OK) return rc;
    }
    if (n_in > 0) {
        const dim3 grid((unsigned)((H + 255) / 256), (unsigned)n_streams);
        if (u8) hipLaunchKernelGGL(chan_hist_kernel<true>, grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL(chan_hist_kernel<false>, grid, dim3(256), 0, st, a);
        SFE_HIP(hipGetLastError());
    }
    return SFE_OK;
}

}  // namespace sfe
