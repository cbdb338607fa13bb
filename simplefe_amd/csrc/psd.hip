// psd.hip -- streaming Welch spectrum estimator (sfe_dsp_psd_*): averaged, windowed periodograms of complex streams.
//
//   b_m    = (m + 1) H - N                                      first sample of segment m (absolute, x[i < 0] = 0)
//   X_m[k] = sum_{n<N} w[n] x[b_m + n] exp(-j 2 pi k n / N)
//   P_m[k] = Re(X_m[k])^2 + Im(X_m[k])^2
//   out_r  = scale * S_r,   S_r = the sum of P_m over m in [rA, (r + 1)A)
//
// The order of that sum is part of the contract (include/sfe_dsp.h): a row's segments go in chunks of C consecutive
// segments counted from the row's first one (C the smallest power of two with C C >= A); a chunk sum is the float32
// left fold of its P_m, S_r the float32 left fold of its chunk sums, both from 0 and ascending.  The host (api_psd.hip)
// counts segments; a call that starts j0 segments into a row and completes q of them is laid out in row-relative
// indices m' in [j0, j0 + q), chunk g' = r' CPR + c (CPR chunks per row) being the segments [r' A + c C, min(.. + C,
// (r' + 1) A)).  Three launches:
//   1. psd_chunk_kernel: one workgroup (256 threads) per chunk piece (the part of one chunk inside the call) of one
//      stream.  Window values and the bin accumulators stay in registers.  ROWS segments at a time (1 from N = 1024
//      on; 4 and 2 for N = 256 and 512, so that every pass has a butterfly for every thread): loads contiguous across
//      lanes, times the window, into LDS; the next batch's loads are issued before this batch's transform; one radix-2
//      pass when log2 N is odd, then forward radix-4 Stockham passes (twiddles from a table of exp(-j 2 pi q / N));
//      each thread squares its bins, fmaf(im, im, re re), and adds them in ascending segment order.  The accumulators
//      start from the carried open-chunk value when the piece starts mid-chunk and go to the other buffer of that pair
//      when the piece ends mid-chunk, else to the call's scratch of chunk sums.
//   2. psd_row_kernel: one thread per (stream, row touched, bin) folds the row's chunk sums that this call completed,
//      starting from the carried open-row value when the row began in an earlier call; a row that completes goes out
//      times scale, one that stays open goes to the other buffer of the open-row pair.  With one chunk per row (A <= 2)
//      S_r = 0 + the chunk sum is the chunk sum: the chunk kernel writes the row itself, no scratch and no row kernel.
//   3. psd_hist_kernel: the N - H samples that end the call, as cf32, into the other buffer of the history pair.
#include "fft16.h"

namespace sfe {

namespace {

constexpr int PSD_THREADS = 256;

struct PsdArgs {
    const void *in;             // call input: stream s at in + s in_stride samples (cf32, or u8 (I,Q) pairs)
    const v2f *hist;            // [n_streams][Hh]: the Hh = N - H samples before the call, oldest first
    v2f *hist_next;             // written by psd_hist_kernel
    const float *win;           // [N]
    const v2f *tw;              // [N]: exp(-j 2 pi q / N)
    const float *chunk_in;      // [n_streams][N]: the open chunk's fold so far
    float *chunk_out;
    const float *row_in;        // [n_streams][N]: the open row's fold so far
    float *row_out;
    float *scratch;             // [n_streams][pieces][N]: the chunk sums this call completes (unused when CPR = 1)
    float *out;
    long long in_stride, out_stride, n_in;
    long long j0, end;          // the call's segments, row-relative: [j0, end), j0 < A
    int H, Hh, A, C, CPR, c0;   // c0 = j0 / C: the chunk of piece 0
    int pieces, rows;           // rows touched: (end - 1) / A + 1
    float scale;
};

__host__ __device__ __forceinline__ long long psd_min(long long x, long long y) { return x < y ? x : y; }
__host__ __device__ __forceinline__ long long psd_max(long long x, long long y) { return x > y ? x : y; }

template <bool U8>
__device__ __forceinline__ v2f psd_load(const void *base, long long i)
{
    if constexpr (U8) {
        const unsigned w = static_cast<const unsigned short *>(base)[i];
        return v2f{u8_to_f32(w & 0xffu), u8_to_f32(w >> 8)};
    } else {
        return static_cast<const v2f *>(base)[i];
    }
}

// the samples of segments t .. t + ROWS - 1 (call-relative) this thread puts into LDS; segments from t_end on are zero
template <int LOGN, int ROWS, bool U8, bool GUARD>
__device__ __forceinline__ void psd_fetch(const PsdArgs &a, const void *in, const v2f *hist, long long t, long long t_end, int tid,
                                          v2f (&x)[ROWS * (1 << LOGN) / PSD_THREADS])
{
    constexpr int N = 1 << LOGN, NE = ROWS * N / PSD_THREADS;
#pragma unroll
    for (int e = 0; e < NE; e++) {
        const int it = e * PSD_THREADS + tid, row = it >> LOGN, n = it & (N - 1);
        const long long i = (t + row + 1) * a.H - N + n;
        if constexpr (GUARD) {
            if (t + row >= t_end) x[e] = v2f{0.0f, 0.0f};
            else if (i < 0) x[e] = hist[a.Hh + i];
            else x[e] = psd_load<U8>(in, i);
        } else {
            x[e] = psd_load<U8>(in, i);
        }
    }
}

// one forward Stockham pass of radix R over ROWS rows of N in LDS: sub-transforms of length Ls = 2^logLs become R Ls long
template <int LOGN, int ROWS, int R>
__device__ __forceinline__ void psd_pass(v2f *V, const v2f *tw, int logLs, int tid)
{
    constexpr int N = 1 << LOGN, NQ = N / R, NI = ROWS * NQ / PSD_THREADS, LOGR = R == 4 ? 2 : 1;
    static_assert(NI * PSD_THREADS == ROWS * NQ, "whole passes per thread");
    const int Ls = 1 << logLs;
    v2f y[NI][R];
#pragma unroll
    for (int e = 0; e < NI; e++) {
        const int it = e * PSD_THREADS + tid, row = it / NQ, j = it % NQ, k = j & (Ls - 1);
        v2f x[R];
#pragma unroll
        for (int r = 0; r < R; r++) x[r] = V[row * N + j + r * NQ];
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
    lds_barrier();
#pragma unroll
    for (int e = 0; e < NI; e++) {
        const int it = e * PSD_THREADS + tid, row = it / NQ, j = it % NQ, k = j & (Ls - 1);
        const int base = ((j >> logLs) << (logLs + LOGR)) + k;
#pragma unroll
        for (int r = 0; r < R; r++) V[row * N + base + r * Ls] = y[e][r];
    }
    lds_barrier();
}

template <int LOGN, bool U8>
__global__ __launch_bounds__(PSD_THREADS) void psd_chunk_kernel(PsdArgs a)
{
    constexpr int N = 1 << LOGN;
    constexpr int ROWS = N >= 1024 ? 1 : 1024 / N;          // segments per batch
    constexpr int NE = ROWS * N / PSD_THREADS;              // samples per thread and batch
    constexpr int NB = N / PSD_THREADS;                     // bins per thread: k = eb 256 + tid
    __shared__ v2f V[ROWS * N];

    const int tid = threadIdx.x;
    const int s = blockIdx.x / a.pieces, p = blockIdx.x % a.pieces;
    const void *in = static_cast<const char *>(a.in) + s * a.in_stride * (U8 ? 2 : 8);
    const v2f *hist = a.hist + (long long)s * a.Hh;

    // the chunk of this piece, and the part of it inside the call (row-relative segment indices)
    const long long g = (long long)a.c0 + p;
    const int r = (int)(g / a.CPR), c = (int)(g % a.CPR);
    const long long cs = (long long)r * a.A + (long long)c * a.C;
    const long long ce = psd_min(cs + a.C, (long long)(r + 1) * a.A);
    const long long lo = psd_max(cs, a.j0), hi = psd_min(ce, a.end);
    const long long t_end = hi - a.j0;                      // call-relative: segment t starts at sample (t + 1) H - N

    float w[NE], acc[NB];
#pragma unroll
    for (int e = 0; e < NE; e++) w[e] = a.win[(e * PSD_THREADS + tid) & (N - 1)];
#pragma unroll
    for (int eb = 0; eb < NB; eb++) acc[eb] = lo > cs ? a.chunk_in[(long long)s * N + eb * PSD_THREADS + tid] : 0.0f;

    // a batch is interior when every segment of it is in the piece and starts at or after the call's first sample
    auto fetch = [&](long long t, v2f (&x)[NE]) {
        if ((t + 1) * a.H - N >= 0 && t + ROWS <= t_end) psd_fetch<LOGN, ROWS, U8, false>(a, in, hist, t, t_end, tid, x);
        else psd_fetch<LOGN, ROWS, U8, true>(a, in, hist, t, t_end, tid, x);
    };

    v2f x[NE];
    long long t = lo - a.j0;
    fetch(t, x);
    for (; t < t_end; t += ROWS) {
#pragma unroll
        for (int e = 0; e < NE; e++) V[e * PSD_THREADS + tid] = x[e] * v2f{w[e], w[e]};
        if (t + ROWS < t_end) fetch(t + ROWS, x);           // in flight over the transform
        lds_barrier();

        int logLs = 0;
        if constexpr (LOGN & 1) {
            psd_pass<LOGN, ROWS, 2>(V, a.tw, 0, tid);
            logLs = 1;
        }
#pragma unroll
        for (; logLs < LOGN; logLs += 2) psd_pass<LOGN, ROWS, 4>(V, a.tw, logLs, tid);

#pragma unroll
        for (int row = 0; row < ROWS; row++) {
            if (ROWS > 1 && t + row >= t_end) break;
#pragma unroll
            for (int eb = 0; eb < NB; eb++) {
                const v2f X = V[row * N + eb * PSD_THREADS + tid];
                acc[eb] = acc[eb] + fmaf(X.y, X.y, X.x * X.x);
            }
        }
        lds_barrier();
    }

    if (hi == ce && a.CPR == 1) {
        // a chunk that is a whole row (A <= 2): S_r = 0 + its sum, the sum itself, so the row goes straight out
        float *dst = a.out + s * a.out_stride + (long long)r * N;
#pragma unroll
        for (int eb = 0; eb < NB; eb++) dst[eb * PSD_THREADS + tid] = a.scale * acc[eb];
        return;
    }
    float *dst = hi < ce ? a.chunk_out + (long long)s * N : a.scratch + ((long long)s * a.pieces + p) * N;
#pragma unroll
    for (int eb = 0; eb < NB; eb++) dst[eb * PSD_THREADS + tid] = acc[eb];
}

template <int LOGN>
__global__ __launch_bounds__(PSD_THREADS) void psd_row_kernel(PsdArgs a)
{
    constexpr int N = 1 << LOGN, BPR = N / PSD_THREADS;     // workgroups per row
    const long long blk = blockIdx.x;
    const int s = (int)(blk / ((long long)a.rows * BPR));
    const long long rb = blk % ((long long)a.rows * BPR);
    const int r = (int)(rb / BPR), k = (int)(rb % BPR) * PSD_THREADS + threadIdx.x;
    const long long row_lo = (long long)r * a.A, row_hi = row_lo + a.A;

    float S = r == 0 && a.j0 > 0 ? a.row_in[(long long)s * N + k] : 0.0f;
    const long long p0 = (long long)s * a.pieces + (long long)r * a.CPR - a.c0;            // piece of the row's chunk 0
    for (int c = r == 0 ? a.c0 : 0; c < a.CPR; c++) {
        if (psd_min(row_lo + (long long)(c + 1) * a.C, row_hi) > a.end) break;    // still open when the call ends
        S = S + a.scratch[(p0 + c) * N + k];
    }
    if (row_hi <= a.end) a.out[s * a.out_stride + (long long)r * N + k] = a.scale * S;
    else a.row_out[(long long)s * N + k] = S;
}

// the Hh samples that end the call (old history followed by the call's input), as cf32, into hist_next
template <bool U8>
__global__ __launch_bounds__(256) void psd_hist_kernel(PsdArgs a)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int s = blockIdx.y;
    if (i >= a.Hh) return;
    const long long src = a.n_in - a.Hh + i;
    const void *in = static_cast<const char *>(a.in) + s * a.in_stride * (U8 ? 2 : 8);
    a.hist_next[(long long)s * a.Hh + i] = src >= 0 ? psd_load<U8>(in, src) : a.hist[(long long)s * a.Hh + a.Hh + src];
}

template <int LOGN>
int psd_launch_n(const PsdArgs &a, int u8, int n_streams, hipStream_t st)
{
    const dim3 grid((unsigned)(a.pieces * (long long)n_streams));
    if (u8) hipLaunchKernelGGL((psd_chunk_kernel<LOGN, true>), grid, dim3(PSD_THREADS), 0, st, a);
    else hipLaunchKernelGGL((psd_chunk_kernel<LOGN, false>), grid, dim3(PSD_THREADS), 0, st, a);
    SFE_HIP(hipGetLastError());
    if (a.CPR > 1) {                        // with one chunk per row the chunk kernel has written the rows itself
        const dim3 rgrid((unsigned)((long long)n_streams * a.rows * ((1 << LOGN) / PSD_THREADS)));
        hipLaunchKernelGGL(psd_row_kernel<LOGN>, rgrid, dim3(PSD_THREADS), 0, st, a);
        SFE_HIP(hipGetLastError());
    }
    return SFE_OK;
}

}  // namespace

// The chunk pieces of a call that starts j0 segments into a row (j0 < A) and completes q >= 1 segments; *rows = the rows
// it touches.  The host sizes the scratch ([n_streams][pieces][N] floats; none when a chunk is a whole row) and the grids with it.
long long psd_pieces(long long j0, long long q, int A, int C, long long *rows)
{
    const long long CPR = (A + C - 1) / C, last = j0 + q - 1;
    if (rows) *rows = last / A + 1;
    return (last / A) * CPR + (last % A) / C - j0 / C + 1;
}

// One call: q = n_in / H segments of every stream, then the row folds, then the history update.  Shapes and buffers are the
// caller's (api_psd.hip) to check: 8 <= logn <= 12, 1 <= H <= N, j0 < A, n_in = q H > 0, scratch of psd_pieces() chunk sums.
int launch_psd(int logn, int u8, const void *in, long long in_stride, const v2f *hist, v2f *hist_next, const float *win, const v2f *tw,
               const float *chunk_in, float *chunk_out, const float *row_in, float *row_out, float *scratch, float *out,
               long long out_stride, long long n_in, int H, int A, int C, long long j0, float scale, int n_streams, hipStream_t st)
{
    const int N = 1 << logn;
    const long long q = n_in / H;
    long long rows = 0;
    const long long pieces = psd_pieces(j0, q, A, C, &rows);
    if (n_streams > 65535 || pieces * n_streams > 0x7fffffffLL || rows * (N / PSD_THREADS) * n_streams > 0x7fffffffLL) {
        set_error("psd_process_stream: call too large for one grid");
        return SFE_EINVAL;
    }
    PsdArgs a{in, hist, hist_next, win, tw, chunk_in, chunk_out, row_in, row_out, scratch, out, in_stride, out_stride, n_in,
              j0, j0 + q, H, N - H, A, C, (A + C - 1) / C, (int)(j0 / C), (int)pieces, (int)rows, scale};
    int rc = SFE_OK;
    switch (logn) {
    case 8: rc = psd_launch_n<8>(a, u8, n_streams, st); break;
    case 9: rc = psd_launch_n<9>(a, u8, n_streams, st); break;
    case 10: rc = psd_launch_n<10>(a, u8, n_streams, st); break;
    case 11: rc = psd_launch_n<11>(a, u8, n_streams, st); break;
    case 12: rc = psd_launch_n<12>(a, u8, n_streams, st); break;
    default: set_error("psd: log2 N = %d has no kernel", logn); return SFE_EINVAL;
    }
    if (rc != SFE_OK) return rc;
    if (a.Hh > 0) {
        const dim3 grid((unsigned)((a.Hh + 255) / 256), (unsigned)n_streams);
        if (u8) hipLaunchKernelGGL(psd_hist_kernel<true>, grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL(psd_hist_kernel<false>, grid, dim3(256), 0, st, a);
        SFE_HIP(hipGetLastError());
    }
    return SFE_OK;
}

}  // namespace sfe
