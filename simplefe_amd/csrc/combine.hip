// combine.hip -- polyphase synthesis filter bank (sfe_dsp_combine_*): M baseband channels at rate 1/D, each interpolated
// by D, shifted up to its own sub-band and summed into one complex stream, in one pass.  The transpose of chan.hip.
//
//   z[i] = sum_m g[i - mD] v_{i mod M}[m],   v_q[m] = sum_k X_k[m] W^{kq},  W = exp(+j 2 pi / M),  D = M or M/2
//
// With i = m'D + r (0 <= r < D) and t = i - mD = jD + r the tap index, v_{i mod M}[m] = u_m[t mod M], where u_m is row
// m of the transform rotated by mD (for D = M/2: by M/2 on odd absolute m, an index permutation), so output column r is
// an FIR over the instants: z[m'D + r] = sum_{j<J} g[jD + r] u_{m'-j}[(jD + r) mod M].
//
// One workgroup (NT = max(256, D) threads) owns G = NT / D segments of `run` consecutive instants of one stream; lane r
// of segment g owns output column r (comb_cs below: two workgroups share the columns of the largest shapes).  It walks
// its instants in chunks of RG rows:
//   1. the chunk's X rows go from global memory to LDS, one padded row of M + 1 per instant: lanes run along m, so a
//      channel's RG instants are one contiguous run (the mirror of chan.hip's step-4 store).
//   2. an unnormalised inverse M-point DFT per row in LDS: self-sorting (Stockham) radix-4 passes, one radix-2 pass
//      first when log2 M is odd, twiddles from a table of exp(+j 2 pi q / M).
//   3. the output FIR, transposed form: acc[j] holds the partial sum of output instant m + j.  Row m adds
//      g[jD + r] u_m[.] to every acc[j]; acc[0] is then complete, goes out, and the delay line shifts by one.  Every
//      output sums its J terms in ascending m, wherever the call, the segment or the chunk starts: cutting a stream at
//      any instant gives the one-call result bit for bit.  A segment starts W0 >= J - 1 rows early to fill its line.
// J = ceil(L / D) rounded up to a power of two >= 8 (the host pads g with zero taps).  The carried history is the
// J - 1 X rows before the call (channel-major, zero at create / reset); combine_hist_kernel writes the next call's
// history into the other buffer of the pair behind the main launch.
// TX10: the output is written in the transmit wire format, 4 floats (2 complex samples) in 5 bytes,
// ((short)(x*511)+512)&0x3FF, as sfe_dsp_tx_f32_to_10bit packs them; the even lane of a pair writes the group.
#include "fft16.h"

namespace sfe {

namespace {

struct CombArgs {
    const v2f *in;              // channel k of stream s at in + (s M + k) in_stride
    const v2f *hist;            // [n_streams][M][Hr]: the Hr instants before the call, oldest first
    v2f *hist_next;             // [n_streams][M][Hr]: written by combine_hist_kernel
    const float *taps;          // [J][D] = g zero-padded to J D
    const v2f *tw;              // [M]: exp(+j 2 pi q / M)
    void *out;                  // F32: stream s at out + s out_stride samples; TX10: at out + s (out_stride / 2) 5 bytes
    long long in_stride, out_stride, n_in, run;   // run: instants per segment, a multiple of RG
    int Hr, parity, tiles, tx10;                  // parity: absolute index of the call's first instant, mod 2
};

// The shape of one instantiation.  CS: workgroups that share an instant's transform, each emitting D / CS of its
// columns -- 2 where one thread per column would need more registers than the workgroup's size allows (M = 1024 with
// J = 32 at D = M, J = 64 at D = M/2).  NT = max(256, D / CS) threads, one per column of G = NT / (D / CS) segments.
// ROWS: transformed rows per chunk (halved at J = 64, to leave the registers to the delay line).
constexpr int comb_cs(int logm, bool half, int logj) { return logm == 10 && logj == (half ? 6 : 5) ? 2 : 1; }
constexpr int comb_cols(int logm, bool half, int logj) { return (half ? (1 << logm) / 2 : 1 << logm) / comb_cs(logm, half, logj); }
constexpr int comb_threads(int logm, bool half, int logj) { return comb_cols(logm, half, logj) > 256 ? comb_cols(logm, half, logj) : 256; }
constexpr int comb_rows(int logm, int logj) { return (logm <= 8 ? 4096 >> logm : 8) >> (logj == 6 ? 1 : 0); }

__device__ __forceinline__ v2f comb_fma(float g, v2f u, v2f acc) { return __builtin_elementwise_fma(v2f{g, g}, u, acc); }

__device__ __forceinline__ unsigned comb_q10(float x) { return (unsigned)((int)(short)(int)(x * 511.0f) + 512) & 0x3FFu; }

// the value held by the odd lane of this lane's pair (DPP quad_perm [1, 1, 3, 3]: plain VALU, every lane active)
__device__ __forceinline__ float comb_pair_odd(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 1 | (1 << 2) | (3 << 4) | (3 << 6), 0xF, 0xF, true));
}

// one Stockham pass of radix R over ROWS rows of M in LDS: sub-transforms of length Ls = 2^logLs become R Ls long
template <int LOGM, int ROWS, int RS, int R, int NT>
__device__ __forceinline__ void comb_pass(v2f *V, const v2f *tw, int logLs, int tid)
{
    constexpr int M = 1 << LOGM, NQ = M / R, NI = ROWS * NQ / NT, LOGR = R == 4 ? 2 : 1;
    static_assert(NI * NT == ROWS * NQ, "whole passes per thread");
    const int Ls = 1 << logLs;
    v2f y[NI][R];
#pragma unroll
    for (int e = 0; e < NI; e++) {
        const int it = e * NT + tid, row = it / NQ, j = it % NQ, k = j & (Ls - 1);
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
        const int it = e * NT + tid, row = it / NQ, j = it % NQ, k = j & (Ls - 1);
        const int base = ((j >> logLs) << (logLs + LOGR)) + k;
#pragma unroll
        for (int r = 0; r < R; r++) V[row * RS + base + r * Ls] = y[e][r];
    }
    lds_barrier();
}

template <int LOGM, bool HALF, int LOGJ>
__global__ __launch_bounds__(comb_threads(LOGM, HALF, LOGJ)) void combine_kernel(CombArgs a)
{
    constexpr int M = 1 << LOGM, D = HALF ? M / 2 : M, J = 1 << LOGJ, CS = comb_cs(LOGM, HALF, LOGJ), DC = D / CS;
    constexpr int NT = comb_threads(LOGM, HALF, LOGJ), G = NT / DC;   // threads; segments per workgroup
    constexpr int ROWS = comb_rows(LOGM, LOGJ), RG = ROWS / G, RS = M + 1;
    constexpr int W0 = (J - 1 + RG - 1) / RG * RG;               // rows a segment reads before its first output
    constexpr int NL = ROWS * M / NT;                            // X samples per thread per chunk
    static_assert(G * DC == NT && RG * G == ROWS && NL * NT == ROWS * M && DC % 2 == 0, "whole rows, segments and pairs");
    __shared__ v2f V[ROWS * RS];

    const int tid = threadIdx.x;
    const int cb = blockIdx.x % CS, s = blockIdx.x / CS / a.tiles, tile = blockIdx.x / CS % a.tiles;
    const int g = tid / DC, r = cb * DC + tid % DC;              // segment, output column
    // per-lane indices are 32-bit within a stream (the host keeps every stream's input and output below 2^31 samples)
    const int run = a.run, n_in = a.n_in, Hr = a.Hr;
    const int seg0 = tile * G;                                   // the workgroup's first segment
    const int ms = (seg0 + g) * run;                             // this lane's first output instant (relative to the call)
    const v2f *in = a.in + (long long)s * M * a.in_stride;
    const v2f *hist = a.hist + (long long)s * M * Hr;
    const int in_stride = a.in_stride;

    float h[J];
#pragma unroll
    for (int j = 0; j < J; j++) h[j] = a.taps[j * D + r];
    v2f acc[J];
#pragma unroll
    for (int j = 0; j < J; j++) acc[j] = v2f{0.0f, 0.0f};

    // chunk c of every segment: rows (seg0 + gg) run - W0 + c RG + t, t < RG; lane tid always loads row t = tid % RG.
    // Every address below is computed again each chunk from a copy of tid the compiler cannot see through, rather than
    // hoisted out of the chunk loop, where the transform's addresses and twiddles alone would hold ~100 registers.
    v2f xr[NL];
    auto load = [&](int c, int tid) {
        const int tl = tid % RG;
        const int m00 = seg0 * run - W0 + c * RG;                // the workgroup's first row of the chunk
        if (m00 >= 0 && m00 + (G - 1) * run + RG <= n_in) {      // every row is a sample of the call (uniform)
#pragma unroll
            for (int e = 0; e < NL; e++) {
                const int it = e * NT + tid, k = (it / RG) % M, gg = it / (RG * M);
                xr[e] = in[k * in_stride + m00 + gg * run + tl];
            }
        } else {
#pragma unroll
            for (int e = 0; e < NL; e++) {
                const int it = e * NT + tid, k = (it / RG) % M, gg = it / (RG * M);
                const int m = m00 + gg * run + tl;
                v2f x = v2f{0.0f, 0.0f};                         // past the call (never an output's term) or before the history
                if (m >= 0 && m < n_in) x = in[k * in_stride + m];
                else if (m < 0 && m >= -Hr) x = hist[k * Hr + Hr + m];
                xr[e] = x;
            }
        }
    };
    const int n_chunks = (W0 + run) / RG;
    for (int c = 0; c < n_chunks; c++) {
        if (seg0 * run - W0 + c * RG >= n_in) break;             // every segment is past the call (uniform)
        int ftid = tid;
        asm volatile("" : "+v"(ftid));
        const int tl = ftid % RG, fr = cb * DC + ftid % DC, fg = ftid / DC;
        load(c, ftid);
#pragma unroll
        for (int e = 0; e < NL; e++) {
            const int it = e * NT + ftid, k = (it / RG) % M, gg = it / (RG * M);
            V[(gg * RG + tl) * RS + k] = xr[e];
        }
        lds_barrier();
        int logLs = 0;
        if constexpr (LOGM & 1) {
            comb_pass<LOGM, ROWS, RS, 2, NT>(V, a.tw, 0, ftid);
            logLs = 1;
        }
#pragma unroll
        for (; logLs < LOGM; logLs += 2) comb_pass<LOGM, ROWS, RS, 4, NT>(V, a.tw, logLs, ftid);

        const int mc = ms - W0 + c * RG;                         // this lane's first row of the chunk
        const bool past_fill = c * RG >= W0;
#pragma unroll
        for (int t = 0; t < RG; t++) {
            const int m = mc + t;
            const v2f *row = V + (fg * RG + t) * RS;
            v2f ue, uo;
            if constexpr (HALF) {
                const int odd = (a.parity + m) & 1;
                ue = row[fr + (odd ? M / 2 : 0)];                 // taps with j even
                uo = row[fr + (odd ? 0 : M / 2)];                 // taps with j odd
            } else {
                ue = row[fr];
                uo = ue;
            }
#pragma unroll
            for (int j = 0; j < J; j++) acc[j] = comb_fma(h[j], (j & 1) ? uo : ue, acc[j]);
            const v2f z = acc[0];
#pragma unroll
            for (int j = 0; j + 1 < J; j++) acc[j] = acc[j + 1];
            acc[J - 1] = v2f{0.0f, 0.0f};
            const bool emit = past_fill && m < n_in;
            const int i = m * D + fr;                             // output sample of the call
            if (a.tx10) {
                const float zx = comb_pair_odd(z.x), zy = comb_pair_odd(z.y);
                if (emit && !(fr & 1)) {
                    const unsigned u0 = comb_q10(z.x), u1 = comb_q10(z.y), u2 = comb_q10(zx), u3 = comb_q10(zy);
                    const unsigned w = ((u0 >> 8) | ((u1 >> 8) << 2) | ((u2 >> 8) << 4) | ((u3 >> 8) << 6)) | ((u0 & 0xFFu) << 8) |
                                       ((u1 & 0xFFu) << 16) | ((u2 & 0xFFu) << 24);
                    unsigned char *o = static_cast<unsigned char *>(a.out) + ((long long)s * (a.out_stride / 2) + (i >> 1)) * 5;
                    __builtin_memcpy(o, &w, 4);
                    o[4] = (unsigned char)u3;
                }
            } else if (emit) {
                (static_cast<v2f *>(a.out) + (long long)s * a.out_stride)[i] = z;
            }
        }
        lds_barrier();
    }
}

// the Hr instants that end the call (old history followed by the call's input), per channel, into hist_next
__global__ __launch_bounds__(256) void combine_hist_kernel(CombArgs a, int M)
{
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    const int s = blockIdx.y;
    if (e >= (long long)M * a.Hr) return;
    const long long k = e / a.Hr, i = e % a.Hr;
    const long long src = a.n_in - a.Hr + i;
    const long long row = (long long)s * M + k;
    a.hist_next[row * a.Hr + i] = src >= 0 ? a.in[row * a.in_stride + src] : a.hist[row * a.Hr + a.Hr + src];
}

template <int LOGM, bool HALF, int LOGJ>
int combine_launch_one(const CombArgs &a, int n_streams, hipStream_t st)
{
    hipLaunchKernelGGL((combine_kernel<LOGM, HALF, LOGJ>), dim3(a.tiles * n_streams * comb_cs(LOGM, HALF, LOGJ)),
                       dim3(comb_threads(LOGM, HALF, LOGJ)), 0, st, a);
    SFE_HIP(hipGetLastError());
    return SFE_OK;
}

// J = 2^logj: 8 ... 32 for D = M (L <= 32 M), 8 ... 64 for D = M / 2
template <int LOGM>
int combine_launch_m(const CombArgs &a, int half, int logj, int n_streams, hipStream_t st)
{
    if (half) {
        switch (logj) {
        case 3: return combine_launch_one<LOGM, true, 3>(a, n_streams, st);
        case 4: return combine_launch_one<LOGM, true, 4>(a, n_streams, st);
        case 5: return combine_launch_one<LOGM, true, 5>(a, n_streams, st);
        case 6: return combine_launch_one<LOGM, true, 6>(a, n_streams, st);
        }
    } else {
        switch (logj) {
        case 3: return combine_launch_one<LOGM, false, 3>(a, n_streams, st);
        case 4: return combine_launch_one<LOGM, false, 4>(a, n_streams, st);
        case 5: return combine_launch_one<LOGM, false, 5>(a, n_streams, st);
        }
    }
    set_error("combine: J = 2^%d taps per output phase has no kernel at D = %s", logj, half ? "M/2" : "M");
    return SFE_EINVAL;
}

}  // namespace

// segments per workgroup of the kernel, and the instants of one segment per chunk (runs are whole chunks)
int combine_segments(int logm, int half, int logj) { return comb_threads(logm, half, logj) / comb_cols(logm, half, logj); }
int combine_chunk_rows(int logm, int half, int logj) { return comb_rows(logm, logj) / combine_segments(logm, half, logj); }

// One call: the combiner over n_in instants of every stream, then the history update.  Shapes and buffers are the
// caller's (api_combine.hip) to check: 2 <= logm <= 10, 3 <= logj <= 5 (6 for D = M/2), Hr = 2^logj - 1, run a
// positive multiple of combine_chunk_rows.
int launch_combine(int logm, int half, int logj, int tx10, const v2f *in, long long in_stride, const v2f *hist, v2f *hist_next,
                   const float *taps, const v2f *tw, void *out, long long out_stride, long long n_in, long long run, int Hr,
                   int parity, int n_streams, hipStream_t st)
{
    CombArgs a{in, hist, hist_next, taps, tw, out, in_stride, out_stride, n_in, run, Hr, parity, 0, tx10};
    const long long per_wg = run * combine_segments(logm, half, logj);
    const long long tiles = (n_in + per_wg - 1) / per_wg;
    if (tiles * n_streams * 2 > 0x7fffffffLL) {
        set_error("combine_process_stream: call too large for one grid");
        return SFE_EINVAL;
    }
    a.tiles = (int)tiles;
    if (n_in <= 0) return SFE_OK;
    int rc = SFE_OK;
    switch (logm) {
    case 2: rc = combine_launch_m<2>(a, half, logj, n_streams, st); break;
    case 3: rc = combine_launch_m<3>(a, half, logj, n_streams, st); break;
    case 4: rc = combine_launch_m<4>(a, half, logj, n_streams, st); break;
    case 5: rc = combine_launch_m<5>(a, half, logj, n_streams, st); break;
    case 6: rc = combine_launch_m<6>(a, half, logj, n_streams, st); break;
    case 7: rc = combine_launch_m<7>(a, half, logj, n_streams, st); break;
    case 8: rc = combine_launch_m<8>(a, half, logj, n_streams, st); break;
    case 9: rc = combine_launch_m<9>(a, half, logj, n_streams, st); break;
    case 10: rc = combine_launch_m<10>(a, half, logj, n_streams, st); break;
    default: set_error("combine: log2 M = %d has no kernel", logm); return SFE_EINVAL;
    }
    if (rc != SFE_OK) return rc;
    const long long elems = (long long)Hr << logm;
    const dim3 grid((unsigned)((elems + 255) / 256), (unsigned)n_streams);
    hipLaunchKernelGGL(combine_hist_kernel, grid, dim3(256), 0, st, a, 1 << logm);
    SFE_HIP(hipGetLastError());
    return SFE_OK;
}

}  // namespace sfe
