// corr.hip -- streaming preamble correlator bank (sfe_dsp_corr_*): K known complex sequences against every stream,
// normalised by the sliding signal energy and reduced to one peak per block before anything leaves the chip.
//
//   c_k[i] = sum_{n<L} conj(s_k[n]) x[i - (L-1) + n]        window ending at absolute sample i (x[i < 0] = 0)
//   e[i]   = sum_{n<L} |x[i - (L-1) + n]|^2
//   m_k[i] = |c_k[i]|^2 / (E_k e[i])  if e[i] > min_energy, else 0
//   block j = samples [jB, (j+1)B): peak_val = max m_k, peak_idx = the smallest offset that attains it
//
// Overlap-save with 4096-point transforms: slot q holds the samples [qV - ov, qV + V), ov = 4096 - V a multiple of 256
// that is >= L - 1, and owns the V outputs of its last V positions.  Calls are multiples of B and B of V, so a slot
// starts at an absolute multiple of V and every value is a function of absolute position only.  Three launches:
//   1. corr_slot_kernel: one workgroup (256 threads) per (stream, slot).  Thread t holds the 16 slot positions
//      n = 256 m + t in registers -- the layout the first and the last radix-4 Stockham pass of a 4096-point transform
//      both take and leave, so samples, spectrum and correlation values never go through LDS outside the four inner
//      exchanges of a transform.  |x|^2 is staged in LDS once, folded from the left and from the right inside every aligned
//      run of 16 positions, and the runs' sums likewise inside every group of 16 runs; e of a window is the float32
//      left fold of: the rest of its first run, the runs and groups between in ascending order, the start of its last
//      run (at most 25 terms, every one a sum of squares: no cancellation, unlike a differenced prefix sum).  The forward transform leaves the spectrum in
//      registers; for each template: spectrum times the template's (conjugated, / 4096; the inverse transform is the
//      forward one of the conjugate) from L2, six passes, |.|^2, the gate and the division, the dense row if asked,
//      and (max, lowest index) over the thread's values, the wave (cross-lane) and the four waves (LDS).  With B = V
//      that is the block's peak; otherwise it goes to the call's table of slot peaks.
//      Templates of up to CORR_DIRECT_MAX samples take the DIRECT form of the same kernel, same slots and same
//      reduction: the slot's samples stay in LDS, c is the sum over n, ascending, of conj(s_k[n]) x[.] in fused
//      multiply-adds and e the left fold of the window's squares.  A transform's rounding error is relative to the RMS
//      of its 4096 samples, and a window of a few samples can lie far below that (at L = 1, m = 1 wherever the gate is
//      open: one weak sample among strong ones misses the 1e-5 bar through the transforms); L K multiply-adds per
//      sample cost no more than the transforms up to there.
//   2. corr_fold_kernel (B > V only): one thread per (stream, template, block) folds the block's B / V slot peaks in
//      ascending order.  Max with lowest-index ties is associative, so the bits are those of any other order.
//   3. corr_hist_kernel: the ov samples that end the call, as cf32, into the other buffer of the history pair.
#include "fft16.h"

namespace sfe {

namespace {

constexpr int CORR_THREADS = 256;
constexpr int CORR_N = 4096;
constexpr int CORR_PER = CORR_N / CORR_THREADS;       // slot positions per thread
constexpr int CORR_DIRECT_MAX = 16;                   // templates up to this length are correlated in the time domain
constexpr int CORR_OV_ROWS = 8;                       // the overlap is at most 8 rows of 256 (L <= 2049)

struct CorrArgs {
    const void *in;             // call input: stream s at in + s in_stride samples (cf32, or u8 (I,Q) pairs)
    const v2f *hist;            // [n_streams][ov]: the ov samples before the call, oldest first
    const v2f *spec;            // [K][4096]: conj(DFT of conj(s_k) reversed) / 4096
    const v2f *tpl;             // [K][L]: the templates themselves (DIRECT)
    const v2f *tw;              // [4096]: exp(-j 2 pi q / 4096)
    const float *energy;        // [K]: E_k
    float *slot_val;            // [n_streams K][slot_stride]: one peak per slot -- the caller's peak arrays when B = V,
    unsigned *slot_idx;         // else the call's table of slot peaks
    float *metric;              // [n_streams K][metric_stride] (DENSE)
    long long in_stride, slot_stride, metric_stride;
    int L, K, V, ov, slots;
    float min_energy;
};

template <bool U8>
__device__ __forceinline__ v2f corr_load(const void *base, long long i)
{
    if constexpr (U8) {
        const unsigned w = static_cast<const unsigned short *>(base)[i];
        return v2f{u8_to_f32(w & 0xffu), u8_to_f32(w >> 8)};
    } else {
        return static_cast<const v2f *>(base)[i];
    }
}

// true when (ov, oi) beats (v, i): the larger value, the lower index among equals
__device__ __forceinline__ bool corr_better(float ov, unsigned oi, float v, unsigned i) { return ov > v || (ov == v && oi < i); }

// LDS position of element i of an array whose aligned runs of 16 are 17 apart: a thread that walks one run per thread
// (17 tid + j) and a wave that reads consecutive elements both meet every bank once
__device__ __forceinline__ int corr_pad(int i) { return i + (i >> 4); }

// One forward radix-4 Stockham pass of the 4096-point transform (psd.hip's, for one row): sub-transforms of length
// 2^LOGLS become four times as long.  The first pass (LOGLS = 0) takes its input from the registers `in` (position
// 256 m + t in in[m]), times conj(in) H when MUL (a product spectrum, conjugated for the inverse transform); the last
// (LOGLS = 10) leaves its output in `out` in the same layout; the passes between go through W.
template <int LOGLS, bool MUL>
__device__ __forceinline__ void corr_pass(const v2f (&in)[CORR_PER], v2f (&out)[CORR_PER], const v2f *H, v2f *W, const v2f *tw, int tid)
{
    constexpr bool FIRST = LOGLS == 0, LAST = LOGLS == 10;
    constexpr int Ls = 1 << LOGLS, NQ = CORR_N / 4;
    v2f y[4][4];
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const int j = e * CORR_THREADS + tid, k = j & (Ls - 1);
        v2f x[4];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            if constexpr (FIRST) {
                if constexpr (MUL) x[r] = cmul_conj(H[(e + 4 * r) * CORR_THREADS + tid], in[e + 4 * r]);
                else x[r] = in[e + 4 * r];
            } else {
                x[r] = W[j + r * NQ];
            }
        }
        if constexpr (!FIRST) {
#pragma unroll
            for (int r = 1; r < 4; r++) x[r] = cmul(x[r], tw[(r * k) << (10 - LOGLS)]);
        }
        const v2f t0 = x[0] + x[2], t1 = x[0] - x[2], t2 = x[1] + x[3], t3 = x[1] - x[3];
        y[e][0] = t0 + t2;
        y[e][1] = add_mj(t1, t3);
        y[e][2] = t0 - t2;
        y[e][3] = add_pj(t1, t3);
    }
    if constexpr (!FIRST) lds_barrier();        // every read of W before anything overwrites it
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const int j = e * CORR_THREADS + tid, k = j & (Ls - 1);
        const int base = ((j >> LOGLS) << (LOGLS + 2)) + k;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            if constexpr (LAST) out[e + 4 * r] = y[e][r];
            else W[base + r * Ls] = y[e][r];
        }
    }
    if constexpr (!LAST) lds_barrier();
}

template <bool MUL>
__device__ __forceinline__ void corr_transform(const v2f (&in)[CORR_PER], v2f (&out)[CORR_PER], const v2f *H, v2f *W, const v2f *tw, int tid)
{
    corr_pass<0, MUL>(in, out, H, W, tw, tid);
    corr_pass<2, false>(in, out, H, W, tw, tid);
    corr_pass<4, false>(in, out, H, W, tw, tid);
    corr_pass<6, false>(in, out, H, W, tw, tid);
    corr_pass<8, false>(in, out, H, W, tw, tid);
    corr_pass<10, false>(in, out, H, W, tw, tid);
}

template <bool U8, bool DENSE, bool DIRECT>
__global__ __launch_bounds__(CORR_THREADS) void corr_slot_kernel(CorrArgs a)
{
    __shared__ v2f W[DIRECT ? CORR_N : CORR_N + CORR_N / 16];     // the transform's 32 KiB; before it, two padded float arrays
    __shared__ float red_v[CORR_THREADS / 64];
    __shared__ unsigned red_i[CORR_THREADS / 64];

    const int tid = threadIdx.x;
    const int s = blockIdx.x / a.slots, q = blockIdx.x % a.slots;
    const void *in = static_cast<const char *>(a.in) + s * a.in_stride * (U8 ? 2 : 8);
    const v2f *hist = a.hist + (long long)s * a.ov;
    const long long first = (long long)q * a.V - a.ov;      // call-relative sample at slot position 0
    const int m0 = a.ov / CORR_THREADS;                     // thread rows m >= m0 hold the slot's outputs

    // ov is a multiple of 256, at most 2048: a row of 256 positions is history as a whole (rows below m0 of the call's
    // first slot) or input as a whole, and rows from CORR_OV_ROWS on are always outputs
    v2f X[CORR_PER];
#pragma unroll
    for (int m = 0; m < CORR_PER; m++) {
        const long long i = first + m * CORR_THREADS + tid;
        if (m < CORR_OV_ROWS && m < m0 && q == 0) X[m] = hist[a.ov + i];
        else X[m] = corr_load<U8>(in, i);
    }

    float ew[CORR_PER];         // the window energy of the thread's positions
    if constexpr (DIRECT) {
        // the slot's samples stay in W; e is the left fold of the window's squares in ascending n.  Overlap rows may
        // reach before the slot: their index wraps, their values are never used
#pragma unroll
        for (int m = 0; m < CORR_PER; m++) W[m * CORR_THREADS + tid] = X[m];
        lds_barrier();
#pragma unroll
        for (int m = 0; m < CORR_PER; m++) ew[m] = 0.0f;
        for (int n = 0; n < a.L; n++) {
#pragma unroll
            for (int m = 0; m < CORR_PER; m++) {
                const v2f x = W[(m * CORR_THREADS + tid - (a.L - 1) + n) & (CORR_N - 1)];
                ew[m] = ew[m] + (x.x * x.x + x.y * x.y);
            }
        }
    } else {
        // The window energies, before W holds the transform.  |x|^2 goes to Ex (padded); one thread per aligned run of
        // 16 positions folds it from the left into Q (Q[i]: the run's first element up to i) and from the right into S
        // (S[i]: i up to the run's last); R16 holds the runs' sums, and one thread per 16 runs does the same over them
        // (Q256, S256, R256).  A window [lo, n] is longer than 16 here, so it is, in this order: S[lo], the runs between
        // -- those of one group of 16 one by one, else S256 of the first, the whole groups between, Q256 of the last --
        // and Q[n].  Every term is a sum of squares: nothing is subtracted.
        __shared__ float Ex[CORR_N + CORR_N / 16];
        __shared__ float R16[CORR_N / 16], Q256[CORR_N / 16], S256[CORR_N / 16], R256[CORR_N / 256];
        float *S = reinterpret_cast<float *>(W), *Q = S + CORR_N + CORR_N / 16;
#pragma unroll
        for (int m = 0; m < CORR_PER; m++) Ex[corr_pad(m * CORR_THREADS + tid)] = X[m].x * X[m].x + X[m].y * X[m].y;
        lds_barrier();
        {
            float p[16], acc = 0.0f;
#pragma unroll
            for (int j = 0; j < 16; j++) {
                p[j] = Ex[17 * tid + j];
                acc = acc + p[j];
                Q[17 * tid + j] = acc;
            }
            R16[tid] = acc;
            acc = 0.0f;
#pragma unroll
            for (int j = 15; j >= 0; j--) {
                acc = acc + p[j];
                S[17 * tid + j] = acc;
            }
        }
        lds_barrier();
        if (tid < 16) {
            float p[16], acc = 0.0f;
#pragma unroll
            for (int j = 0; j < 16; j++) {
                p[j] = R16[16 * tid + j];
                acc = acc + p[j];
                Q256[16 * tid + j] = acc;
            }
            R256[tid] = acc;
            acc = 0.0f;
#pragma unroll
            for (int j = 15; j >= 0; j--) {
                acc = acc + p[j];
                S256[16 * tid + j] = acc;
            }
        }
        lds_barrier();
        float *En = Ex;         // the squares have been read: the energies take their place, unpadded
#pragma unroll 1
        for (int m = m0; m < CORR_PER; m++) {
            const int n = m * CORR_THREADS + tid, lo = n - a.L + 1;
            const int b0 = (lo >> 4) + 1, b1 = (n >> 4) - 1;        // the whole runs inside the window
            float e = S[corr_pad(lo)];
            if (b0 <= b1) {
                if ((b0 >> 4) == (b1 >> 4)) {
                    for (int b = b0; b <= b1; b++) e = e + R16[b];
                } else {
                    e = e + S256[b0];
                    for (int g = (b0 >> 4) + 1; g < (b1 >> 4); g++) e = e + R256[g];
                    e = e + Q256[b1];
                }
            }
            En[n] = e + Q[corr_pad(n)];
        }
#pragma unroll
        for (int m = 0; m < CORR_PER; m++) ew[m] = En[m * CORR_THREADS + tid];       // the thread's own: no barrier between
    }
    // the thread's own, as the divisor's second factor: +infinity where the gate is shut (the quotient is then +0), NaN in
    // the rows that are overlap, not output (never a maximum)
    float en[CORR_PER];
#pragma unroll
    for (int m = 0; m < CORR_PER; m++) {
        en[m] = m < CORR_OV_ROWS && m < m0 ? __builtin_nanf("") : ew[m] > a.min_energy ? ew[m] : __builtin_inff();
    }
    if constexpr (!DIRECT) {
        lds_barrier();
        corr_transform<false>(X, X, nullptr, W, a.tw, tid);
    }

    for (int k = 0; k < a.K; k++) {
        v2f c[CORR_PER];
        if constexpr (DIRECT) {
            // c = the sum over n, ascending, of conj(s_k[n]) x[. - (L-1) + n], each term two fused multiply-adds per part
#pragma unroll
            for (int m = 0; m < CORR_PER; m++) c[m] = v2f{0.0f, 0.0f};
            const v2f *tpl = a.tpl + (long long)k * a.L;
            for (int n = 0; n < a.L; n++) {
                const v2f t = tpl[n];
#pragma unroll
                for (int m = 0; m < CORR_PER; m++) {
                    const v2f x = W[(m * CORR_THREADS + tid - (a.L - 1) + n) & (CORR_N - 1)];
                    c[m] = v2f{fmaf(t.y, x.y, fmaf(t.x, x.x, c[m].x)), fmaf(-t.y, x.x, fmaf(t.x, x.y, c[m].y))};
                }
            }
        } else {
            corr_transform<true>(X, c, a.spec + (long long)k * CORR_N, W, a.tw, tid);
        }
        const float Ek = a.energy[k];
        const long long row = (long long)s * a.K + k;
        float *dense = DENSE ? a.metric + row * a.metric_stride + (long long)q * a.V + tid : nullptr;
        float v[CORR_PER];
#pragma unroll
        for (int m = 0; m < CORR_PER; m++) {
            v[m] = (c[m].x * c[m].x + c[m].y * c[m].y) / (Ek * en[m]);
            if constexpr (DENSE) {
                if (m >= CORR_OV_ROWS || m >= m0) dense[(m - m0) * CORR_THREADS] = v[m];
            }
        }
        // row CORR_OV_ROWS is an output row whatever the overlap: start there, the index settles the order
        float bv = v[CORR_OV_ROWS];
        unsigned bi = (unsigned)((CORR_OV_ROWS - m0) * CORR_THREADS + tid);
#pragma unroll
        for (int m = 0; m < CORR_PER; m++) {
            const unsigned i = (unsigned)((m - m0) * CORR_THREADS + tid);
            if (m != CORR_OV_ROWS && corr_better(v[m], i, bv, bi)) {
                bv = v[m];
                bi = i;
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const float ov = __shfl_xor(bv, off);
            const unsigned oi = __shfl_xor(bi, off);
            if (corr_better(ov, oi, bv, bi)) {
                bv = ov;
                bi = oi;
            }
        }
        if ((tid & 63) == 0) {
            red_v[tid >> 6] = bv;
            red_i[tid >> 6] = bi;
        }
        lds_barrier();
        if (tid == 0) {
#pragma unroll
            for (int w = 1; w < CORR_THREADS / 64; w++) {
                if (corr_better(red_v[w], red_i[w], bv, bi)) {
                    bv = red_v[w];
                    bi = red_i[w];
                }
            }
            a.slot_val[row * a.slot_stride + q] = bv;
            a.slot_idx[row * a.slot_stride + q] = bi;
        }
        // thread 0 has read red_* before anything writes it again: the transform's barriers, or this one
        if constexpr (DIRECT) lds_barrier();
    }
}

// block j of row (stream, template): the fold of its spb slot peaks, ascending
__global__ __launch_bounds__(256) void corr_fold_kernel(const float *part_val, const unsigned *part_idx, long long slots, float *peak_val,
                                                        unsigned *peak_idx, long long peak_stride, long long rows, long long blocks,
                                                        int spb, int V)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= rows * blocks) return;
    const long long row = t / blocks, j = t % blocks;
    const float *pv = part_val + row * slots + j * spb;
    const unsigned *pi = part_idx + row * slots + j * spb;
    float bv = pv[0];
    unsigned bi = pi[0];
    for (int r = 1; r < spb; r++) {
        const float v = pv[r];
        const unsigned i = (unsigned)r * (unsigned)V + pi[r];
        if (corr_better(v, i, bv, bi)) {
            bv = v;
            bi = i;
        }
    }
    peak_val[row * peak_stride + j] = bv;
    peak_idx[row * peak_stride + j] = bi;
}

// the ov samples that end the call (n_in >= V >= ov: all of them are input), as cf32, into the next call's history
template <bool U8>
__global__ __launch_bounds__(256) void corr_hist_kernel(const void *in0, long long in_stride, long long n_in, int ov, v2f *hist_next)
{
    const int i = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
    if (i >= ov) return;
    const void *in = static_cast<const char *>(in0) + s * in_stride * (U8 ? 2 : 8);
    hist_next[(long long)s * ov + i] = corr_load<U8>(in, n_in - ov + i);
}

}  // namespace

// One call: n_in = blocks B samples of every stream.  Shapes and buffers are the caller's (api_corr.hip) to check:
// V = 4096 - ov, ov a multiple of 256 with L - 1 <= ov <= 2048, B a multiple of V, n_in > 0 a multiple of B below 2^31,
// part_* of n_streams K (n_in / V) entries when B > V.
int launch_corr(int u8, const void *in, long long in_stride, const v2f *hist, v2f *hist_next, const v2f *spec, const v2f *tpl, const v2f *tw,
                const float *energy, float *peak_val, unsigned *peak_idx, long long peak_stride, float *part_val, unsigned *part_idx,
                float *metric, long long metric_stride, long long n_in, int L, int K, int V, long long B, float min_energy,
                int n_streams, hipStream_t st)
{
    const long long slots = n_in / V, blocks = n_in / B, rows = (long long)n_streams * K;
    if (n_streams > 65535 || slots * n_streams > 0x7fffffffLL || rows * blocks > 0x7fffffffLL) {
        set_error("corr_process_stream: call too large for one grid");
        return SFE_EINVAL;
    }
    const int ov = CORR_N - V, spb = (int)(B / V);
    const CorrArgs a{in, hist, spec, tpl, tw, energy, spb == 1 ? peak_val : part_val, spb == 1 ? peak_idx : part_idx, metric, in_stride,
                     spb == 1 ? peak_stride : slots, metric_stride, L, K, V, ov, (int)slots, min_energy};
    const dim3 grid((unsigned)(slots * n_streams));
    const dim3 block(CORR_THREADS);
    switch ((u8 ? 4 : 0) | (metric ? 2 : 0) | (L <= CORR_DIRECT_MAX ? 1 : 0)) {
    case 0: hipLaunchKernelGGL((corr_slot_kernel<false, false, false>), grid, block, 0, st, a); break;
    case 1: hipLaunchKernelGGL((corr_slot_kernel<false, false, true>), grid, block, 0, st, a); break;
    case 2: hipLaunchKernelGGL((corr_slot_kernel<false, true, false>), grid, block, 0, st, a); break;
    case 3: hipLaunchKernelGGL((corr_slot_kernel<false, true, true>), grid, block, 0, st, a); break;
    case 4: hipLaunchKernelGGL((corr_slot_kernel<true, false, false>), grid, block, 0, st, a); break;
    case 5: hipLaunchKernelGGL((corr_slot_kernel<true, false, true>), grid, block, 0, st, a); break;
    case 6: hipLaunchKernelGGL((corr_slot_kernel<true, true, false>), grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL((corr_slot_kernel<true, true, true>), grid, block, 0, st, a); break;
    }
    SFE_HIP(hipGetLastError());
    if (spb > 1) {
        hipLaunchKernelGGL(corr_fold_kernel, dim3((unsigned)((rows * blocks + 255) / 256)), dim3(256), 0, st, part_val, part_idx, slots,
                           peak_val, peak_idx, peak_stride, rows, blocks, spb, V);
        SFE_HIP(hipGetLastError());
    }
    if (ov > 0) {
        const dim3 hgrid((unsigned)((ov + 255) / 256), (unsigned)n_streams);
        if (u8) hipLaunchKernelGGL(corr_hist_kernel<true>, hgrid, dim3(256), 0, st, in, in_stride, n_in, ov, hist_next);
        else hipLaunchKernelGGL(corr_hist_kernel<false>, hgrid, dim3(256), 0, st, in, in_stride, n_in, ov, hist_next);
        SFE_HIP(hipGetLastError());
    }
    return SFE_OK;
}

}  // namespace sfe
