// eig.hip -- symmetric eigen-decomposition / MUSIC direction finder (sfe_dsp_eig_*): per (output row of the covariance
// estimator, band) the eigenvalues and eigenvectors of the real 2S x 2S Gram matrix, the MUSIC null spectrum of B scan
// steering vectors and the E leading eigenvectors as the real 2E x 2S matrix the beamformer multiplies by
// (include/sfe_dsp.h states the law; api_eig.hip is its float64 twin and shares eig.h's scalar pieces).
//
// ONE WORKGROUP (256 lanes) PER PROBLEM, everything between the read of G and the stores in LDS and registers.  The
// method is the two-sided cyclic Jacobi method in round-robin order: it is right for every finite symmetric matrix --
// singular and indefinite ones too, which a one-sided method on G^ itself is not (it cannot tell +lambda from -lambda).
//   read     the upper triangle of G, one 2 x 2 block (s <= t) per lane and step; the structure of the mode is applied on
//            the way in and both triangles of G^ are stored (the same bits twice).  The strict lower triangle of G is
//            never addressed.  The largest |G^| bit pattern is folded by an LDS atomic max (order-free): a pattern of an
//            infinity or a NaN fails the problem, the exponent of any other scales G^ by a power of two into [1, 2) --
//            exactly -- so that no rotation overflows and the stopping threshold is a constant.
//            The linear mode stores the S x S Hermitian Z it is the realification of, (re, im) pairs, both triangles (an
//            odd S gets a phantom index of zeros), and rotates that: a quarter of the blocks, and eigenvectors that
//            come in exact (u(w), u(jw)) pairs however the eigenvalues cluster.
//   step     n / 2 disjoint pairs (linear: ceil(S / 2), complex: the coupling's phase is taken out of row and column q).  The first n / 2 lanes compute their pair's rotation from its three entries and
//            finish its diagonal block (app - t apq, aqq + t apq, the coupling exactly zero); barrier; every other 2 x 2
//            block (pairs a != b) is J_a^T X J_b on its own four words -- no lane reads what another writes -- with lanes
//            along b, so the words of one instruction lie in one row of A; and the rows p, q of V^T are rotated, lanes
//            along the row; barrier.  Two barriers per step, n - 1 steps per sweep.
//   stop     after the first sweep in which no coupling exceeded 2^-27 of the scale (all were still rotated), or at 30.
//   finish   rank sort of the diagonal (descending, ties by index), per vector its norm and the sign of its largest
//            component, V^T normalised in place; the eigen-beams; the null spectrum, a beam per wave and pass: lane e
//            holds the noise eigenvectors e and e + 64 (linear: the complex one e), walks their rows (odd stride: no bank conflict) against the
//            beam's steering vector (one address per wave), and the three sums of Q meet in a fixed six-step butterfly.
// The order of every sum is a function of n and D alone: never of M, B, the row, an address or a stride.
#include <cfloat>

#include "eig.h"

namespace sfe {

namespace {

// the sum over the 64 lanes of a wave, the same bits in all of them; every lane of the wave must be active
__device__ inline float sum64(float v)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = v + __shfl_xor(v, m);
    return v;
}

template <bool WL>
__global__ __launch_bounds__(256) void eig_kernel(EigArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int S = a.S, B = a.B, E = a.E, D = a.D, n = 2 * S, ldv = n + 1;
    const int m = eig_order(S, WL), h = m / 2;              // indices of the pair order (linear, odd S: one phantom), pairs of a step
    const int nv = WL ? n : S;                              // eigenvectors kept: rows of V^T
    float *A = reinterpret_cast<float *>(smem);             // WL: [n][n]; linear: Z [m][m] (re, im)
    float *Vt = A + (WL ? n * n : 2 * m * m);               // [m][n + 1]: row i is (the vector that becomes) eigenvector i
    float *rc = Vt + m * ldv, *rs = rc + 64, *rwr = rs + 64, *rwi = rwr + 64;   // the step's rotations
    int *rp = reinterpret_cast<int *>(rwi + 64), *rq = rp + 64;
    float *nrm = reinterpret_cast<float *>(rq + 64);        // [128]: the signed norm of row i of V^T
    int *ord = reinterpret_cast<int *>(nrm + 128);          // [128]: ord[r] is the row of V^T that holds eigenvector r
    unsigned *flags = reinterpret_cast<unsigned *>(ord + 128);      // [0]: max |G^| bits; [1 + sweep]: a coupling above the threshold
    const int words = WL ? n * n : 2 * m * m;
    const size_t row = blockIdx.x, band = blockIdx.y;
    const float *G = a.gram + band * (size_t)a.in_stride + row * (size_t)(n * n);
    float *val = a.values + row * (size_t)a.values_stride + band * (size_t)n;
    float *nul = a.null_spec ? a.null_spec + row * (size_t)a.null_stride + band * (size_t)B : nullptr;
    float *vec = a.vectors ? a.vectors + row * (size_t)a.vectors_stride + band * (size_t)(2 * E * n) : nullptr;

    if (tid < 64) flags[tid] = 0u;
    if (!WL && m != S)                                      // the phantom index: a zero row and column
        for (int t = tid; t < m; t += 256) {
            A[2 * (S * m + t)] = A[2 * (S * m + t) + 1] = 0.0f;
            A[2 * (t * m + S)] = A[2 * (t * m + S) + 1] = 0.0f;
        }
    __syncthreads();

    // ---- read + structure: block (s, t), s <= t, of the upper triangle and its mirror
    unsigned top = 0u;
    for (int p = tid; p < S * S; p += 256) {
        const int s = p / S, t = p - s * S;
        if (s > t) continue;
        const float *g = G + (size_t)(2 * s) * n + 2 * t;
        const float g00 = g[0], g01 = g[1], g11 = g[n + 1];
        const float g10 = s == t ? g01 : g[n];              // the diagonal block's lower entry is its upper one's mirror
        if (WL) {
            A[(2 * s) * n + 2 * t] = A[(2 * t) * n + 2 * s] = g00;
            A[(2 * s) * n + 2 * t + 1] = A[(2 * t + 1) * n + 2 * s] = g01;
            A[(2 * s + 1) * n + 2 * t] = A[(2 * t) * n + 2 * s + 1] = g10;
            A[(2 * s + 1) * n + 2 * t + 1] = A[(2 * t + 1) * n + 2 * s + 1] = g11;
            const unsigned m0 = __float_as_uint(g00) & 0x7fffffffu, m1 = __float_as_uint(g01) & 0x7fffffffu;
            const unsigned m2 = __float_as_uint(g10) & 0x7fffffffu, m3 = __float_as_uint(g11) & 0x7fffffffu;
            top = max(max(top, max(m0, m1)), max(m2, m3));
        } else {
            const float hh = 0.5f * (g00 + g11), xx = 0.5f * (g10 - g01);   // Z[s][t] = G^[2s][2t] + j G^[2s+1][2t]
            A[2 * (s * m + t)] = A[2 * (t * m + s)] = hh;
            A[2 * (t * m + s) + 1] = -xx;
            A[2 * (s * m + t) + 1] = s == t ? 0.0f : xx;    // (the diagonal's is +-0 or, from an infinity, a NaN)
            top = max(top, max(__float_as_uint(hh) & 0x7fffffffu, __float_as_uint(xx) & 0x7fffffffu));
        }
    }
    atomicMax(&flags[0], top);
    __syncthreads();
    top = flags[0];
    bool ok = top < 0x7f800000u;                            // every entry of G^ finite; the same word for every lane
    // the scale: 2^ex <= max |G^| < 2^(ex + 1), subnormal values included (a zero matrix keeps its zeros)
    const int ex = !top ? 0 : (top >> 23) ? (int)(top >> 23) - 127 : (31 - __clz((int)top)) - 149;

    int sweeps = 0;
    if (ok) {
        for (int p = tid; p < words; p += 256) A[p] = ldexpf(A[p], -ex);
        for (int p = tid; p < m * n; p += 256) {
            const int i = p / n, j = p - i * n;
            Vt[i * ldv + j] = (WL ? i == j : 2 * i == j) ? 1.0f : 0.0f;
        }
        __syncthreads();
        const float thr = ldexpf(1.0f, EIG_TOL_EXP);
        const int da = 256 / h, db = 256 - da * h, dva = 256 / n, dvj = 256 - dva * n;
        ok = false;
        for (; sweeps < EIG_MAX_SWEEPS && !ok; sweeps++) {
            for (int r = 0; r < m - 1; r++) {
                if (tid < h) {
                    int p, q;
                    eig_pair(m, r, tid, &p, &q);
                    float c, s, t;
                    if (WL) {
                        const float app = A[p * n + p], apq = A[p * n + q], aqq = A[q * n + q];
                        eig_rotation(app, apq, aqq, &c, &s, &t);
                        if (apq != 0.0f) {
                            A[p * n + p] = fmaf(-t, apq, app);
                            A[q * n + q] = fmaf(t, apq, aqq);
                            A[p * n + q] = A[q * n + p] = 0.0f;
                            if (fabsf(apq) > thr) flags[1 + sweeps] = 1u;
                        }
                    } else {
                        const float app = A[2 * (p * m + p)], aqq = A[2 * (q * m + q)];
                        const float zr = A[2 * (p * m + q)], zi = A[2 * (p * m + q) + 1];
                        float wr, wi, mod;
                        eig_rotation_c(app, zr, zi, aqq, &c, &s, &t, &wr, &wi, &mod);
                        rwr[tid] = wr, rwi[tid] = wi;
                        if (mod != 0.0f) {
                            A[2 * (p * m + p)] = fmaf(-t, mod, app);
                            A[2 * (q * m + q)] = fmaf(t, mod, aqq);
                            A[2 * (p * m + q)] = A[2 * (p * m + q) + 1] = 0.0f;
                            A[2 * (q * m + p)] = A[2 * (q * m + p) + 1] = 0.0f;
                            if (mod > thr) flags[1 + sweeps] = 1u;
                        }
                    }
                    rc[tid] = c, rs[tid] = s, rp[tid] = p, rq[tid] = q;
                }
                __syncthreads();
                {
                    int ia = tid / h, ib = tid - ia * h;
                    for (; ia < h; ia += da, ib += db) {
                        if (ib >= h) {
                            ib -= h;
                            if (++ia >= h) break;
                        }
                        if (ia == ib) continue;
                        if (WL) {
                            const int pa = rp[ia] * n, qa = rq[ia] * n, pb = rp[ib], qb = rq[ib];
                            float x00 = A[pa + pb], x01 = A[pa + qb], x10 = A[qa + pb], x11 = A[qa + qb];
                            eig_block(ia > ib, rc[ia], rs[ia], rc[ib], rs[ib], &x00, &x01, &x10, &x11);
                            A[pa + pb] = x00, A[pa + qb] = x01, A[qa + pb] = x10, A[qa + qb] = x11;
                        } else {
                            const int pa = rp[ia] * m, qa = rq[ia] * m, pb = rp[ib], qb = rq[ib];
                            v2f *Z = reinterpret_cast<v2f *>(A);
                            const v2f z00 = Z[pa + pb], z01 = Z[pa + qb], z10 = Z[qa + pb], z11 = Z[qa + qb];
                            float x[8] = {z00.x, z00.y, z01.x, z01.y, z10.x, z10.y, z11.x, z11.y};
                            eig_block_c(ia > ib, rc[ia], rs[ia], rwr[ia], rwi[ia], rc[ib], rs[ib], rwr[ib], rwi[ib], x);
                            Z[pa + pb] = v2f{x[0], x[1]}, Z[pa + qb] = v2f{x[2], x[3]};
                            Z[qa + pb] = v2f{x[4], x[5]}, Z[qa + qb] = v2f{x[6], x[7]};
                        }
                    }
                }
                if (WL) {
                    int ia = tid / n, j = tid - ia * n;
                    for (; ia < h; ia += dva, j += dvj) {
                        if (j >= n) {
                            j -= n;
                            if (++ia >= h) break;
                        }
                        float *vp = Vt + rp[ia] * ldv + j, *vq = Vt + rq[ia] * ldv + j;
                        float x = *vp, y = *vq;
                        eig_rot2(rc[ia], rs[ia], &x, &y);
                        *vp = x, *vq = y;
                    }
                } else {                                    // a complex component (two words) per item
                    const int dsa = 256 / S, dsj = 256 - dsa * S;
                    int ia = tid / S, j = tid - ia * S;
                    for (; ia < h; ia += dsa, j += dsj) {
                        if (j >= S) {
                            j -= S;
                            if (++ia >= h) break;
                        }
                        float *vp = Vt + rp[ia] * ldv + 2 * j, *vq = Vt + rq[ia] * ldv + 2 * j;
                        float xr = vp[0], xi = vp[1], yr = vq[0], yi = vq[1];
                        eig_cmul(rwr[ia], -rwi[ia], &yr, &yi);
                        eig_rot2(rc[ia], rs[ia], &xr, &yr);
                        eig_rot2(rc[ia], rs[ia], &xi, &yi);
                        vp[0] = xr, vp[1] = xi, vq[0] = yr, vq[1] = yi;
                    }
                }
                __syncthreads();
            }
            ok = flags[1 + sweeps] == 0u;                   // written before the step's barriers: the same word for every lane
        }
    }

    const float qnan = __builtin_nanf("");
    if (!ok) {                                              // G^ not finite, or the sweep limit: the stated fallback
        if (tid < n) val[tid] = qnan;
        if (nul)
            for (int b = tid; b < B; b += 256) nul[b] = qnan;
        if (vec)
            for (int e = tid; e < 2 * E * n; e += 256) vec[e] = (e / n == e % n) ? 1.0f : 0.0f;
        if (a.status && tid == 0) a.status[row * (size_t)a.status_stride + band] = 1;
        return;
    }

    // ---- order, sign and norm
    if (tid < nv) {
        const int dstep = WL ? n + 1 : 2 * (m + 1);         // from one diagonal entry to the next
        const float di = A[tid * dstep];
        int rank = 0;
        for (int j = 0; j < nv; j++) {
            const float dj = A[j * dstep];
            rank += (dj > di || (dj == di && j < tid)) ? 1 : 0;
        }
        ord[rank] = tid;
        if (WL) val[rank] = ldexpf(di, ex);
        else val[2 * rank] = val[2 * rank + 1] = ldexpf(di, ex);
        const float *v = Vt + tid * ldv;
        float ss = 0.0f, big = 0.0f, at = 1.0f;
        for (int j = 0; j < n; j++) {
            const float x = v[j];
            ss = fmaf(x, x, ss);
            if (fabsf(x) > big) big = fabsf(x), at = x;     // the first of the largest
        }
        const float nn = sqrtf(ss);
        nrm[tid] = at < 0.0f ? -nn : nn;
    }
    __syncthreads();
    for (int p = tid; p < nv * n; p += 256) {
        const int i = p / n, j = p - i * n;
        Vt[i * ldv + j] = Vt[i * ldv + j] / nrm[i];
    }
    __syncthreads();

    // ---- eigen-beams: rows 2e, 2e + 1 of the beamformer's real matrix
    if (vec)
        for (int p = tid; p < 2 * E * n; p += 256) {
            const int r = p / n, j = p - r * n;
            float v;
            if (WL) {
                v = Vt[ord[r] * ldv + j];
            } else if (!(r & 1)) {
                v = Vt[ord[r >> 1] * ldv + j];
            } else {                                        // row 2e+1 is row 2e's rotation: [2s] = -[2s+1], [2s+1] = [2s]
                const float w = Vt[ord[r >> 1] * ldv + (j ^ 1)];
                v = (j & 1) ? w : -w;
            }
            vec[p] = v;
        }

    // ---- null spectrum: a beam per wave and pass.  Widely linear: lane e holds the noise eigenvectors D + e and
    // D + e + 64.  Linear: the complex noise eigenvector D / 2 + e, which stands for u(w) and u(jw): Q = |w^H a|^2 I.
    if (nul) {
        const int first = WL ? D : D / 2, r0 = first + lane, r1 = r0 + 64;
        const float *v0 = Vt + ord[r0 < nv ? r0 : nv - 1] * ldv, *v1 = Vt + ord[r1 < nv ? r1 : nv - 1] * ldv;
        for (int b = wave; b < B; b += 4) {
            const float *st = a.steer + (band * (size_t)B + b) * (size_t)n;
            float x0 = 0.0f, y0 = 0.0f, x1 = 0.0f, y1 = 0.0f, aa = 0.0f;
            for (int s = 0; s < S; s++) {
                const float re = st[2 * s], im = st[2 * s + 1];     // u(a) = (re, im), u(ja) = (-im, re)
                const float p0 = v0[2 * s], q0 = v0[2 * s + 1];
                aa = fmaf(im, im, fmaf(re, re, aa));
                x0 = fmaf(q0, im, fmaf(p0, re, x0));
                y0 = fmaf(q0, re, fmaf(-p0, im, y0));
                if (WL) {
                    const float p1 = v1[2 * s], q1 = v1[2 * s + 1];
                    x1 = fmaf(q1, im, fmaf(p1, re, x1));
                    y1 = fmaf(q1, re, fmaf(-p1, im, y1));
                }
            }
            if (r0 >= nv) x0 = y0 = 0.0f;                   // idle slots recomputed the last vector: they add nothing
            if (r1 >= nv) x1 = y1 = 0.0f;
            float lmin;
            if (WL) {
                const float q00 = sum64(fmaf(x1, x1, x0 * x0)), q11 = sum64(fmaf(y1, y1, y0 * y0)), q01 = sum64(fmaf(x1, y1, x0 * y0));
                const float mid = 0.5f * (q00 + q11), d = 0.5f * (q00 - q11);
                lmin = mid - sqrtf(fmaf(d, d, q01 * q01));
            } else {
                lmin = sum64(fmaf(y0, y0, x0 * x0));
            }
            if (lane == 0) nul[b] = fmaxf(lmin, 0.0f) / aa;
        }
    }
    if (a.status && tid == 0) a.status[row * (size_t)a.status_stride + band] = 0;
}

}  // namespace

int launch_eig(const EigArgs &a, int widely_linear, long long n_rows, hipStream_t st)
{
    const dim3 grid((unsigned)n_rows, (unsigned)a.M);
    const size_t lds = eig_lds_bytes(a.S, widely_linear);  // widely linear: above 64 KB from S = 45 on
    if (widely_linear) {
        if (lds > 65536) SFE_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&eig_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(eig_kernel<true>, grid, dim3(256), lds, st, a);
    } else {
        if (lds > 65536) SFE_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&eig_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(eig_kernel<false>, grid, dim3(256), lds, st, a);
    }
    SFE_HIP(hipGetLastError());
    return SFE_OK;
}

}  // namespace sfe
