// mvdr.hip -- adaptive beamforming weight solver (sfe_dsp_mvdr_*): per (output row of the covariance estimator, band) one
// regularised MVDR problem on the real 2S x 2S Gram matrix, solved where the matrix lies and written as the real
// 2B x 2S matrix the beamformer multiplies by (include/sfe_dsp.h states the law; api_mvdr.hip is its float64 twin).
//
// ONE WORKGROUP (256 lanes) PER PROBLEM, everything between the read of G and the store of R in LDS and registers:
//   read     the upper triangle of G, one 2 x 2 block (s <= t) per lane and step; the structure of the mode is applied on
//            the way in and the result stored as the LOWER triangle of G^ (its mirror), packed row-major: 33 KB for
//            n = 128 where the padded square would be 66 KB.  The strict lower triangle of G is never addressed.
//   load     trace(G^) is the left fold of the diagonal in index order (every lane folds it: LDS broadcasts);
//            lambda = fmaf(load_rel, trace / n, load_abs).
//   factor   right-looking Cholesky on the VECTOR ALU, a column per step: the pivot is read by every lane (so a failed
//            pivot ends the loop for the whole workgroup at once), the scaled column is kept twice -- in the triangle
//            and, contiguous, in col[] -- and the trailing update A[i][j] = fmaf(-col[i], col[j], A[i][j]) runs a row
//            per wave, consecutive j on consecutive lanes (consecutive LDS words).  Two barriers per column.
//   solve    right-hand sides go through in passes of 32 "slots": eight per wave, EIGHT LANES PER SLOT.  Lane q of a
//            slot owns the elements i = q (mod 8) of its vector (in LDS, but lane-private: [i][slot of the wave], one
//            word per lane and step, conflict-free) and sums the terms p = q (mod 8) of every dot product in ascending
//            order from zero; the eight partial sums meet in a fixed three-step butterfly of DPP moves (lanes ^1, ^2,
//            mirror of 8).  Forward substitution reads row i of L (consecutive words), back substitution column i.
//            No barrier: nothing a wave writes here is read by another.
//   finish   q = u.z (linear) or the 2 x 2 Q and its explicit inverse (widely linear: the two slots of a beam sit in
//            lanes l and l ^ 8 and trade values by DPP row rotation), the rows of R, the power; a beam whose q / det Q is
//            not finite and positive takes its rows of the fallback table instead, a problem whose factorisation failed
//            takes all of them.  (S = 1, widely linear: A2 is square and R = A2^-1 in closed form, see there.)
// The order of every sum is a function of n alone: never of M, B, the slot, the row, an address or a stride.
// A blocked factorisation on the matrix pipe (16-wide panels, v_mfma_f32_16x16x4_f32 trailing updates as in cov.hip)
// is the known next step; DESIGN.md 4.14 says why this one was built first and what bounds it.
//
// The second kernel here rewrites a beamformer's fragment table from a device matrix (sfe_dsp_mvdr_load_beam).
#include <cfloat>

#include "mvdr.h"
// beam.h's index helpers are plain host C++; this file also calls beam_frag_at from a kernel
#pragma clang force_cuda_host_device begin
#include "beam.h"
#pragma clang force_cuda_host_device end

namespace sfe {

namespace {

constexpr int DPP_XOR1 = 0xB1, DPP_XOR2 = 0x4E, DPP_HALF_MIRROR = 0x141, DPP_ROR8 = 0x128;

template <int CTRL>
__device__ inline float dpp(float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}

// the sum of the eight lanes of a slot, the same bits in all eight; every lane of the wave must be active
__device__ inline float sum8(float v)
{
    v = v + dpp<DPP_XOR1>(v);
    v = v + dpp<DPP_XOR2>(v);
    return v + dpp<DPP_HALF_MIRROR>(v);
}

__device__ inline int tri(int i, int j) { return i * (i + 1) / 2 + j; }
__device__ inline bool pos_finite(float v) { return v > 0.0f && v <= FLT_MAX; }

template <bool WL>
__global__ __launch_bounds__(256) void mvdr_kernel(MvdrArgs a)
{
    __shared__ float Lp[MVDR_TRI];                      // G^, then L below its diagonal
    __shared__ float dg[MVDR_MAX_N], col[MVDR_MAX_N];   // L's diagonal; the column of the current step
    __shared__ float Y[4][MVDR_MAX_N * 8];              // per wave: [i][slot]
    __shared__ int beam_failed;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int S = a.S, B = a.B, n = 2 * S;
    const size_t row = blockIdx.x, band = blockIdx.y;
    const float *G = a.gram + band * (size_t)a.in_stride + row * (size_t)(n * n);
    float *Rout = a.R + row * (size_t)a.out_stride + band * (size_t)(2 * B * n);
    const float *fb = a.fallback + band * (size_t)(2 * B * n);

    // ---- read + structure: block (s, t), s <= t, of the upper triangle into the lower triangle of G^
    for (int p = tid; p < S * S; p += 256) {
        const int s = p / S, t = p - s * S;
        if (s > t) continue;
        const float *g = G + (size_t)(2 * s) * n + 2 * t;
        const float g00 = g[0], g01 = g[1], g11 = g[n + 1];
        const float g10 = s == t ? g01 : g[n];          // the diagonal block's lower entry is its upper one's mirror
        if (WL) {
            Lp[tri(2 * t, 2 * s)] = g00;
            Lp[tri(2 * t + 1, 2 * s)] = g01;
            if (s < t) Lp[tri(2 * t, 2 * s + 1)] = g10;
            Lp[tri(2 * t + 1, 2 * s + 1)] = g11;
        } else {
            const float h = 0.5f * (g00 + g11), x = 0.5f * (g10 - g01);     // x = G^[2s+1][2t] = -G^[2s][2t+1]
            Lp[tri(2 * t, 2 * s)] = h;
            Lp[tri(2 * t + 1, 2 * s)] = -x;
            if (s < t) Lp[tri(2 * t, 2 * s + 1)] = x;
            Lp[tri(2 * t + 1, 2 * s + 1)] = h;
        }
    }
    if (tid == 0) beam_failed = 0;
    __syncthreads();

    // ---- loading
    float tr = 0.0f;
    for (int i = 0; i < n; i++) tr = tr + Lp[tri(i, i)];
    const float lam = fmaf(a.load_rel, tr / (float)n, a.load_abs);
    __syncthreads();
    if (tid < n) Lp[tri(tid, tid)] = Lp[tri(tid, tid)] + lam;
    __syncthreads();

    // ---- factor
    bool ok = true;
    for (int k = 0; k < n; k++) {
        const float d = Lp[tri(k, k)];                  // the same word for every lane: the branch is uniform
        if (!pos_finite(d)) {
            ok = false;
            break;
        }
        const float lkk = sqrtf(d);
        const int ic = k + 1 + tid;
        if (ic < n) {
            const float v = Lp[tri(ic, k)] / lkk;
            Lp[tri(ic, k)] = v;
            col[ic] = v;
        }
        if (tid == 0) dg[k] = lkk;
        __syncthreads();
        // n <= 128: a lane has at most two columns of a row, the same two for every row of the step
        const int j0 = k + 1 + lane, j1 = j0 + 64;
        const float c0 = j0 < n ? col[j0] : 0.0f, c1 = j1 < n ? col[j1] : 0.0f;
#pragma unroll 4
        for (int i = k + 1 + wave; i < n; i += 4) {
            const float ci = -col[i];
            float *Ai = Lp + tri(i, 0);
            if (j0 <= i) Ai[j0] = fmaf(ci, c0, Ai[j0]);
            if (j1 <= i) Ai[j1] = fmaf(ci, c1, Ai[j1]);
        }
        __syncthreads();
    }

    const float qnan = __builtin_nanf("");
    if (!ok) {                                          // every beam falls back
        for (int e = tid; e < 2 * B * n; e += 256) Rout[e] = fb[e];
        if (a.power)
            for (int b = tid; b < B; b += 256) a.power[row * (size_t)a.power_stride + band * (size_t)B + b] = qnan;
        if (a.status && tid == 0) a.status[row * (size_t)a.status_stride + band] = 1;
        return;
    }

    // ---- solve + finish
    const int r = lane >> 3, q = lane & 7, nslot = WL ? 2 * B : B;
    float *Yw = Y[wave] + r;
    for (int s0 = 0; s0 < nslot; s0 += MVDR_SLOTS) {
        const int slot_raw = s0 + wave * 8 + r;
        const bool valid = slot_raw < nslot;
        const int slot = valid ? slot_raw : nslot - 1;  // idle slots redo the last one (every lane stays active) and store nothing
        const int b = WL ? slot >> 1 : slot, part = WL ? slot & 1 : 0;
        const float *st = a.steer + (band * (size_t)B + b) * (size_t)n;
        // u(a) is the steering vector's own floats; u(ja)[2s] = -Im a_s, u(ja)[2s+1] = Re a_s
        auto u_at = [&](int i) { return part ? ((i & 1) ? st[i - 1] : -st[i + 1]) : st[i]; };

        if (WL && S == 1) {
            // A2 is square: the constraint alone fixes R = A2^-1, the conventional beamformer, whatever G is, and
            // Q^-1 = A2^-1 G^ A2^-T has the trace of G^ over |a|^2.  The general path would reach the same R through a
            // cancellation that costs cond(G) roundings.
            if (valid && q < 2) Rout[2 * (2 * b + part) + q] = fb[2 * (2 * b + part) + q];
            if (a.power && valid && q == 0 && part == 0)
                a.power[row * (size_t)a.power_stride + band * (size_t)B + b] = fmaf(2.0f, lam, tr) / fmaf(st[1], st[1], st[0] * st[0]);
            continue;
        }
        for (int i = q; i < n; i += 8) Yw[i * 8] = u_at(i);
        for (int i = 0; i < n; i++) {                   // L y = u
            const float *Li = Lp + tri(i, 0);
            float acc = 0.0f;
#pragma unroll 4
            for (int p = q; p < i; p += 8) acc = fmaf(Li[p], Yw[p * 8], acc);
            acc = sum8(acc);
            if ((i & 7) == q) Yw[i * 8] = (Yw[i * 8] - acc) / dg[i];
        }
        for (int i = n - 1; i >= 0; i--) {              // L^T z = y
            float acc = 0.0f;
#pragma unroll 4
            for (int p = i + 1 + ((q - i - 1) & 7); p < n; p += 8) acc = fmaf(Lp[tri(p, i)], Yw[p * 8], acc);
            acc = sum8(acc);
            if ((i & 7) == q) Yw[i * 8] = (Yw[i * 8] - acc) / dg[i];
        }

        float ds = 0.0f, dc = 0.0f;                     // u . z of the slot; u . z of the beam's other slot
        for (int i0 = 0; i0 < n; i0 += 8) {
            const int i = i0 + q;
            const float z = i < n ? Yw[i * 8] : 0.0f, u = i < n ? u_at(i) : 0.0f;
            ds = fmaf(u, z, ds);
            if (WL) dc = fmaf(u, dpp<DPP_ROR8>(z), dc);
        }
        ds = sum8(ds);
        float scale_own, scale_other = 0.0f, den, pw;
        if (WL) {
            dc = sum8(dc);
            const float other_ds = dpp<DPP_ROR8>(ds), other_dc = dpp<DPP_ROR8>(dc);
            const float q00 = part ? other_ds : ds, q11 = part ? ds : other_ds, q01 = part ? other_dc : dc;
            den = fmaf(q00, q11, -(q01 * q01));
            scale_own = part ? q00 : q11;               // row 2b: (Q11 z0 - Q01 z1) / det, row 2b+1: (Q00 z1 - Q01 z0) / det
            scale_other = q01;
            pw = (q00 + q11) / den;
        } else {
            den = ds;
            scale_own = 1.0f;
            pw = 2.0f / den;
        }
        const bool good = pos_finite(den);
        if (!good && valid) beam_failed = 1;
        const size_t row0 = (size_t)(2 * b + part) * n;
        for (int i0 = 0; i0 < n; i0 += 8) {
            const int i = i0 + q;
            const float z = i < n ? Yw[i * 8] : 0.0f;
            float v;
            if (WL) v = fmaf(scale_own, z, -(scale_other * dpp<DPP_ROR8>(z))) / den;
            else v = z / den;
            if (!valid || i >= n) continue;
            if (WL) {
                Rout[row0 + i] = good ? v : fb[row0 + i];
            } else {                                    // row 2b+1 is row 2b's rotation: [2s] = -[2s+1], [2s+1] = [2s]
                const int ir = i ^ 1;
                Rout[row0 + i] = good ? v : fb[row0 + i];
                Rout[row0 + n + ir] = good ? ((i & 1) ? -v : v) : fb[row0 + n + ir];
            }
        }
        if (a.power && valid && q == 0 && part == 0) a.power[row * (size_t)a.power_stride + band * (size_t)B + b] = good ? pw : qnan;
    }
    __syncthreads();
    if (a.status && tid == 0) a.status[row * (size_t)a.status_stride + band] = beam_failed ? 2 : 0;
}

__global__ __launch_bounds__(256) void mvdr_load_beam_kernel(const float *R, float *frag, int S, int B, int KS, int nf)
{
    const int f = (int)(blockIdx.x * 256 + threadIdx.x);
    if (f >= nf) return;
    const size_t band = blockIdx.y;
    int row, col;
    beam_frag_at((f >> 6) / KS, (f >> 6) % KS, f & 63, &row, &col);
    float v = 0.0f;
    if (row < 2 * B && col < 2 * S) v = R[(band * 2 * B + row) * (size_t)(2 * S) + col];
    frag[band * (size_t)nf + f] = v;
}

}  // namespace

int launch_mvdr(const MvdrArgs &a, int widely_linear, long long n_rows, hipStream_t st)
{
    const dim3 grid((unsigned)n_rows, (unsigned)a.M);
    if (widely_linear) hipLaunchKernelGGL(mvdr_kernel<true>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(mvdr_kernel<false>, grid, dim3(256), 0, st, a);
    SFE_HIP(hipGetLastError());
    return SFE_OK;
}

int launch_mvdr_load_beam(const float *R, float *frag, int S, int B, int M, hipStream_t st)
{
    const int KS = 2 * beam_kp(S), nf = (int)beam_frag_floats(S, B);
    hipLaunchKernelGGL(mvdr_load_beam_kernel, dim3((unsigned)((nf + 255) / 256), (unsigned)M), dim3(256), 0, st, R, frag, S, B, KS, nf);
    SFE_HIP(hipGetLastError());
    return SFE_OK;
}

}  // namespace sfe
