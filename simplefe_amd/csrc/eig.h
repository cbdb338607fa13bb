// eig.h -- what eig.hip (the kernel) and api_eig.hip (the handle and its float64 twin) share: the limits of a shape, the
// LDS layout of a problem, the launcher, and the scalar pieces of the Jacobi method -- the pair order, the rotation of a
// pair and the update of a 2 x 2 block, real (widely-linear mode) and complex (linear mode) -- written once for float (the
// kernel) and double (the host plan).  No kernels here.
#pragma once
#include <cmath>

#include "common.h"

namespace sfe {

constexpr int EIG_MAX_IN = 64, EIG_MAX_BEAMS = 64, EIG_MAX_BANDS = 1024;         // the beamformer's own limits (beam.h)
constexpr long long EIG_MAX_WEIGHTS = 1LL << 20;                                  // M max(B, E, 1) S
constexpr int EIG_MAX_SWEEPS = 30;
// A sweep in which no coupling exceeded 2^EIG_TOL_EXP times the scale (the power of two at or below the largest |G^|
// entry) was the last: every coupling it met was still rotated away.  The float64 plan uses 2^EIG_TOL_EXP_HOST.
constexpr int EIG_TOL_EXP = -27, EIG_TOL_EXP_HOST = -56;
// The linear mode's G^ is the realification of the S x S Hermitian Z = H + jX (Z[s][t] = G^[2s][2t] + j G^[2s+1][2t]) and is
// decomposed as such, by complex rotations: eigenvectors then come in exact (u(w), u(jw)) pairs.  An odd S gets a phantom
// last index whose row and column are zero: it is never rotated (its couplings are exactly zero) and never reported.
constexpr int eig_order(int S, int wl) { return wl ? 2 * S : S + (S & 1); }      // indices the pair order runs over
// LDS of one problem, in 4-byte words.  Widely linear: A [n][n], V^T [n][n + 1].  Linear: Z [Sp][Sp] (re, im), V^T
// [Sp][n + 1], a complex eigenvector w per row as u(w).  (The odd stride keeps lanes that walk different rows on different
// banks.)  Then c, s, w, p, q of the step's pairs [6][64], the signed norm of every vector [128], the sorted order [128]
// and the flags [64]: the largest |G^| bits, then a word per sweep.
constexpr int EIG_TAIL_WORDS = 6 * 64 + 128 + 128 + 64;
constexpr size_t eig_lds_bytes(int S, int wl)
{
    const size_t n = 2 * (size_t)S, m = (size_t)eig_order(S, wl);
    return ((wl ? n * n : 2 * m * m) + m * (n + 1) + EIG_TAIL_WORDS) * 4;
}

struct EigArgs {
    const float *gram;          // row j of band k at gram + k in_stride + j n^2
    const float *steer;         // [M][B][S] (re, im), or null with B = 0
    float *values;              // row j, band k at values + j values_stride + k n
    float *null_spec;           // or null: + j null_stride + k B + b
    float *vectors;             // or null: + j vectors_stride + k 2E n
    int *status;                // or null: + j status_stride + k
    long long in_stride, values_stride, null_stride, vectors_stride, status_stride;
    int S, B, E, M, D;
};

// One call: n_rows >= 1 rows of every band, one workgroup per (row, band).  Shapes and buffers are the caller's
// (api_eig.hip) to check.
int launch_eig(const EigArgs &a, int widely_linear, long long n_rows, hipStream_t st);

// ---- the method's scalar pieces
__host__ __device__ inline float eig_fma(float a, float b, float c) { return fmaf(a, b, c); }
__host__ __device__ inline double eig_fma(double a, double b, double c) { return fma(a, b, c); }
__host__ __device__ inline float eig_sqrt(float a) { return sqrtf(a); }
__host__ __device__ inline double eig_sqrt(double a) { return sqrt(a); }

// Round-robin order: step r = 0 .. n - 2 of a sweep pairs all n indices (n even) into n / 2 disjoint pairs a = 0 ..
// n / 2 - 1, and the n - 1 steps meet every pair of indices once.  p < q.
__host__ __device__ inline void eig_pair(int n, int r, int a, int *p, int *q)
{
    const int m = n - 1;
    int i = a == 0 ? m : r + a, j = a == 0 ? r : r - a + m;
    if (a != 0 && i >= m) i -= m;
    if (a != 0 && j >= m) j -= m;
    *p = i < j ? i : j;
    *q = i < j ? j : i;
}

// The rotation J = [[c, s], [-s, c]] that annihilates the coupling apq of the pair (p, q) in J^T A J, by the smaller
// root t of t^2 + 2 theta t - 1 = 0; a pair whose coupling is exactly zero is not rotated.
template <class T>
__host__ __device__ inline void eig_rotation(T app, T apq, T aqq, T *c, T *s, T *t)
{
    if (apq == T(0)) {
        *c = T(1), *s = T(0), *t = T(0);
        return;
    }
    const T theta = (aqq - app) / (T(2) * apq);             // an overflow to infinity gives t = 0
    const T at = theta < T(0) ? -theta : theta;
    const T tt = T(1) / (at + eig_sqrt(eig_fma(theta, theta, T(1))));
    *t = theta < T(0) ? -tt : tt;
    *c = T(1) / eig_sqrt(eig_fma(*t, *t, T(1)));
    *s = *t * *c;
}

// (x, y) <- (c x - s y, s x + c y): a column pair under J, a row pair under J^T, two rows of V^T
template <class T>
__host__ __device__ inline void eig_rot2(T c, T s, T *x, T *y)
{
    const T u = eig_fma(c, *x, -(s * *y)), v = eig_fma(s, *x, c * *y);
    *x = u, *y = v;
}

// The 2 x 2 block X of rows (pa, qa), columns (pb, qb), a != b, under J_a^T X J_b.  The block of the lower triangle
// (a > b) is computed as the transpose of its mirror, operation for operation, so that A stays symmetric bit for bit.
template <class T>
__host__ __device__ inline void eig_block(bool lower, T ca, T sa, T cb, T sb, T *x00, T *x01, T *x10, T *x11)
{
    if (!lower) {
        eig_rot2(cb, sb, x00, x01);
        eig_rot2(cb, sb, x10, x11);
        eig_rot2(ca, sa, x00, x10);
        eig_rot2(ca, sa, x01, x11);
    } else {
        eig_rot2(ca, sa, x00, x10);
        eig_rot2(ca, sa, x01, x11);
        eig_rot2(cb, sb, x00, x01);
        eig_rot2(cb, sb, x10, x11);
    }
}

// ---- the linear mode's complex forms.  A complex number is its (re, im) pair of scalars.
template <class T>
__host__ __device__ inline void eig_cmul(T wr, T wi, T *xr, T *xi)          // x <- w x
{
    const T r = eig_fma(*xr, wr, -(*xi * wi)), i = eig_fma(*xr, wi, *xi * wr);
    *xr = r, *xi = i;
}

// The rotation of the complex pair (p, q) with coupling z = Z[p][q] = m w, |w| = 1: U = diag(1, conj w) J with J the real
// rotation above for the coupling m, so that U^H Z U has Z[p][q] = 0.  m by the scaled form, which cannot underflow;
// z exactly zero: no rotation.
template <class T>
__host__ __device__ inline void eig_rotation_c(T app, T zr, T zi, T aqq, T *c, T *s, T *t, T *wr, T *wi, T *m)
{
    const T ar = zr < T(0) ? -zr : zr, ai = zi < T(0) ? -zi : zi;
    const T big = ar > ai ? ar : ai, small = ar > ai ? ai : ar;
    if (big == T(0)) {
        *c = T(1), *s = T(0), *t = T(0), *wr = T(1), *wi = T(0), *m = T(0);
        return;
    }
    const T ratio = small / big;
    *m = big * eig_sqrt(eig_fma(ratio, ratio, T(1)));
    *wr = zr / *m, *wi = zi / *m;
    eig_rotation(app, *m, aqq, c, s, t);
}

// A 2 x 2 complex block X of rows (pa, qa), columns (pb, qb), a != b, under U_a^H X U_b: column qb times conj w_b, the
// columns rotated by (cb, sb), row qa times w_a, the rows rotated by (ca, sa).  x[0 .. 7] = x00, x01, x10, x11 as (re, im).
// The block of the lower triangle (a > b) is computed as the conjugate transpose of its mirror, operation for operation,
// so that Z stays Hermitian bit for bit.
template <class T>
__host__ __device__ inline void eig_block_c(bool lower, T ca, T sa, T war, T wai, T cb, T sb, T wbr, T wbi, T *x)
{
    if (lower) {        // X^H, and the two pairs trade places
        T u;
        u = x[2], x[2] = x[4], x[4] = u;
        u = x[3], x[3] = x[5], x[5] = u;
        x[1] = -x[1], x[3] = -x[3], x[5] = -x[5], x[7] = -x[7];
        u = ca, ca = cb, cb = u;
        u = sa, sa = sb, sb = u;
        u = war, war = wbr, wbr = u;
        u = wai, wai = wbi, wbi = u;
    }
    eig_cmul(wbr, -wbi, &x[2], &x[3]);
    eig_cmul(wbr, -wbi, &x[6], &x[7]);
    eig_rot2(cb, sb, &x[0], &x[2]);
    eig_rot2(cb, sb, &x[1], &x[3]);
    eig_rot2(cb, sb, &x[4], &x[6]);
    eig_rot2(cb, sb, &x[5], &x[7]);
    eig_cmul(war, wai, &x[4], &x[5]);
    eig_cmul(war, wai, &x[6], &x[7]);
    eig_rot2(ca, sa, &x[0], &x[4]);
    eig_rot2(ca, sa, &x[1], &x[5]);
    eig_rot2(ca, sa, &x[2], &x[6]);
    eig_rot2(ca, sa, &x[3], &x[7]);
    if (lower) {
        T u;
        u = x[2], x[2] = x[4], x[4] = u;
        u = x[3], x[3] = x[5], x[5] = u;
        x[1] = -x[1], x[3] = -x[3], x[5] = -x[5], x[7] = -x[7];
    }
}

}  // namespace sfe
