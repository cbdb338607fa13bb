// qam.hip -- the kernels of the QAM mapper and soft demapper (sfe_dsp_qam_*, include/sfe_dsp.h): rows of coded bytes to rows
// of cf32 constellation points, and rows of cf32 equalised symbols to rows of float32 max-log soft values, by the law of
// qam_law.h.  Compiled with -ffp-contract=off (build.py: EXACT_SOURCES); the host plan (api_qam.hip) compiles the same
// header, and the two give the same bits.
//
// Both are streaming kernels: demap moves 8 + 4 bps bytes a symbol, map bps / 8 + 8.  One launch per call; a workgroup of
// 256 lanes takes one tile of QAM_TILE symbols of one row, the call's tiles x rows workgroups laid along x and then y.  No
// atomics, no scratch, nothing carried.
//   demap   a lane owns a group of G symbols, G = 4, 2, 1, 2, 1 for bps = 1, 2, 4, 6, 8, so that its G bps floats are whole
//           16-byte vectors (bps = 6: two symbols, three vectors).  Where the row's output lies on a 16-byte boundary the
//           lane stores vectors, else the same floats one by one; likewise its G symbols come as 16-byte loads where the
//           row's input lies so and G > 1, else as 8-byte ones.  Which form: one scalar branch per row.  The last group of a
//           row may be short: it goes float by float.  At bps = 6 and 8 a lane's floats are three and two vectors, and stored
//           from the lane each store of the wave would leave gaps of 32 or 16 bytes (measured: 43 - 59 % of the copy ceiling
//           where bps = 4 reaches 87 %); a wave all of whose lanes hold whole groups passes its floats through its own stretch
//           of LDS instead and stores 1 KiB in one piece per instruction.
//           The soft values are qam_axis's: the law's e_v, every one, and its minima through partial minima the bits share
//           -- 136 vector operations a symbol at bps = 8 where the statement has about 200.  The level
//           table arrives by value and is read at constant places: scalar registers.
//   csi     the workgroup first writes the weights scale |H|^2 of the residues q mod csi_period its tile meets -- at most
//           min(QAM_TILE, csi_period) of them -- into LDS, one gather of the csi row per tile; a symbol then reads its
//           weight from LDS.  The residue of a group's first symbol comes from one float product and a correction (the
//           numbers are below 2^13), the next ones by counting.
//   perm    demap scatters: a lane stores float t of its group at perm[t], read coalesced.  map gathers: the lane reads
//           perm[t] for its symbols' positions and picks each coded bit from the row's bytes.
//   map     a lane owns two symbols, one 16-byte store where the row's output lies so, else two 8-byte ones.  Without perm
//           its 2 bps bits are a window of at most three bytes of the row.  The level table sits in LDS (the words are
//           picked by a runtime index).
#include "qam.h"

namespace sfe {
namespace {

struct QamWork {
    unsigned row, q0, nq;       // the row, the tile's first symbol, its symbols
};

__device__ __forceinline__ bool qam_work(const QamArgs &a, QamWork *w)
{
    const unsigned id = blockIdx.y * gridDim.x + blockIdx.x;
    if (id >= a.n_wg) return false;
    w->row = id / a.tiles;
    w->q0 = (id - w->row * a.tiles) * QAM_TILE;
    w->nq = min(QAM_TILE, a.n_sym - w->q0);
    return true;
}

template <int BPS, bool CSI, bool PERM>
__global__ __launch_bounds__(QAM_THREADS) void qam_demap_kernel(QamArgs a)
{
    constexpr int G = BPS == 1 ? 4 : (BPS == 2 || BPS == 6) ? 2 : 1, F = G * BPS, ITER = (int)QAM_TILE / (QAM_THREADS * G);
    static_assert(F % 4 == 0 && ITER * QAM_THREADS * G == (int)QAM_TILE, "whole vectors per lane, whole tiles per workgroup");
    constexpr bool TRANSPOSE = !PERM && F > 4;       // a lane's floats are more than one vector: its stores would leave gaps
    __shared__ float s_w[CSI ? QAM_MAX_CSI_PERIOD : 1];
    __shared__ __attribute__((aligned(16))) float s_t[TRANSPOSE ? QAM_THREADS * F : 4];
    QamWork k;
    if (!qam_work(a, &k)) return;
    const unsigned tid = threadIdx.x, P = a.csi_period;
    const v2f *__restrict__ in = static_cast<const v2f *>(a.in) + (size_t)k.row * (size_t)a.in_stride;
    float *__restrict__ out = static_cast<float *>(a.out) + (size_t)k.row * (size_t)a.out_stride;
    unsigned base = 0;
    float inv_p = 0.0f;
    if (CSI) {
        base = k.q0 % P;
        inv_p = 1.0f / (float)P;
        const v2f *__restrict__ csi = a.csi + (size_t)k.row * (size_t)a.csi_stride;
        const unsigned cnt = min(k.nq, P);
        for (unsigned j = tid; j < cnt; j += QAM_THREADS) {
            unsigned i = base + j;
            if (i >= P) i -= P;
            const v2f h = csi[a.csi_index[i]];
            s_w[i] = qam_weight(QamC{h.x, h.y}, a.scale);
        }
        lds_barrier();
    }
    const bool wide_out = !PERM && (reinterpret_cast<uintptr_t>(out) & 15u) == 0;
    const bool wide_in = G > 1 && (reinterpret_cast<uintptr_t>(in) & 15u) == 0;

#pragma unroll
    for (int it = 0; it < ITER; it++) {
        const unsigned j0 = ((unsigned)it * QAM_THREADS + tid) * G;
        if (j0 >= k.nq) break;
        const unsigned q = k.q0 + j0, cnt = min((unsigned)G, k.nq - j0);
        const bool whole = cnt == (unsigned)G;
        QamC z[G];
        if (G > 1 && whole && wide_in) {
#pragma unroll
            for (int g = 0; g < G; g += 2) {
                const v4f v = *reinterpret_cast<const v4f *>(in + q + g);
                z[g] = QamC{v.x, v.y};
                z[g + 1] = QamC{v.z, v.w};
            }
        } else {
#pragma unroll
            for (int g = 0; g < G; g++) {
                z[g] = QamC{0.0f, 0.0f};
                if ((unsigned)g < cnt) {
                    const v2f v = in[q + g];
                    z[g] = QamC{v.x, v.y};
                }
            }
        }
        unsigned res = 0;
        if (CSI) {      // (base + j0) mod P: the quotient by one float product, right to within one
            const unsigned idx = base + j0;
            const unsigned qd = (unsigned)((float)idx * inv_p);
            int r0 = (int)idx - (int)(qd * P);
            if (r0 < 0) r0 += (int)P;
            else if (r0 >= (int)P) r0 -= (int)P;
            res = (unsigned)r0;
        }
        float r[F];
#pragma unroll
        for (int g = 0; g < G; g++) {
            float w = a.scale;
            if (CSI) {
                w = s_w[res];
                res = res + 1 == P ? 0 : res + 1;
            }
            qam_symbol<BPS>(a.lev, z[g], w, r + g * BPS);
        }
        const unsigned t0 = q * BPS;
        const unsigned jw = ((unsigned)it * QAM_THREADS + (tid & ~63u)) * G;       // the first symbol of the wave's 64 groups
        if (TRANSPOSE && wide_out && jw + 64u * G <= k.nq) {
            // every lane of the wave has a whole group: the wave's 64 F floats go through its own stretch of LDS, so that each
            // store is 1 KiB in one piece.  A wave's LDS operations complete in the order it issues them: no barrier.
            float *mine = s_t + (tid & ~63u) * F;
            const unsigned lane = tid & 63u;
#pragma unroll
            for (int v = 0; v < F / 4; v++)
                *reinterpret_cast<v4f *>(mine + lane * F + 4 * v) = v4f{r[4 * v], r[4 * v + 1], r[4 * v + 2], r[4 * v + 3]};
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            float *dst = out + (k.q0 + jw) * BPS;
#pragma unroll
            for (int v = 0; v < F / 4; v++)
                *reinterpret_cast<v4f *>(dst + (v * 64 + lane) * 4) = *reinterpret_cast<const v4f *>(mine + (v * 64 + lane) * 4);
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        } else if (wide_out && whole) {
#pragma unroll
            for (int v = 0; v < F / 4; v++)
                *reinterpret_cast<v4f *>(out + t0 + 4 * v) = v4f{r[4 * v], r[4 * v + 1], r[4 * v + 2], r[4 * v + 3]};
        } else {
#pragma unroll
            for (int f = 0; f < F; f++)
                if ((unsigned)f < cnt * BPS) out[PERM ? a.perm[t0 + f] : t0 + f] = r[f];
        }
    }
}

template <int BPS, bool PERM>
__global__ __launch_bounds__(QAM_THREADS) void qam_map_kernel(QamArgs a)
{
    constexpr int G = 2, ITER = (int)QAM_TILE / (QAM_THREADS * G);
    constexpr unsigned MASK = (1u << BPS) - 1u;
    __shared__ float s_lev[QAM_MAX_WORDS];
    QamWork k;
    if (!qam_work(a, &k)) return;
    const unsigned tid = threadIdx.x;
    {
        float v = a.lev[0];
#pragma unroll
        for (int w = 1; w < QAM_MAX_WORDS; w++) v = tid == (unsigned)w ? a.lev[w] : v;
        if (tid < (unsigned)QAM_MAX_WORDS) s_lev[tid] = v;
    }
    lds_barrier();
    const uint8_t *__restrict__ in = static_cast<const uint8_t *>(a.in) + (size_t)k.row * (size_t)a.in_stride;
    v2f *__restrict__ out = static_cast<v2f *>(a.out) + (size_t)k.row * (size_t)a.out_stride;
    const bool wide = (reinterpret_cast<uintptr_t>(out) & 15u) == 0;

#pragma unroll
    for (int it = 0; it < ITER; it++) {
        const unsigned j0 = ((unsigned)it * QAM_THREADS + tid) * G;
        if (j0 >= k.nq) break;
        const unsigned q = k.q0 + j0, cnt = min((unsigned)G, k.nq - j0), t0 = q * BPS;
        unsigned bits = 0;          // the 2 bps bits of the two symbols, the first one's first bit the most significant
        if (PERM) {
#pragma unroll
            for (int f = 0; f < G * BPS; f++)
                if ((unsigned)f < cnt * BPS) bits |= qam_coded_bit(in, a.perm[t0 + f]) << (G * BPS - 1 - f);
        } else {
            const unsigned byte0 = t0 >> 3, off = t0 & 7u, need = off + cnt * BPS;      // bits of the window that are the row's
            unsigned win = 0;
#pragma unroll
            for (int b = 0; b < 3; b++)
                if (8u * b < need) win |= (unsigned)in[byte0 + b] << (16 - 8 * b);
            bits = (win >> (24 - G * BPS - off)) & ((1u << (G * BPS)) - 1u);
        }
        const QamC p0 = qam_point(s_lev, BPS, bits >> BPS), p1 = qam_point(s_lev, BPS, bits & MASK);
        if (wide && cnt == 2) {
            *reinterpret_cast<v4f *>(out + q) = v4f{p0.r, p0.i, p1.r, p1.i};
        } else {
            out[q] = v2f{p0.r, p0.i};
            if (cnt == 2) out[q + 1] = v2f{p1.r, p1.i};
        }
    }
}

inline dim3 qam_grid(unsigned n_wg)
{
    const unsigned gx = n_wg < QAM_GRID_X ? n_wg : QAM_GRID_X;
    return dim3(gx, (n_wg + gx - 1) / gx);
}

template <int BPS>
int qam_demap_go(const QamArgs &a, hipStream_t st)
{
    const dim3 grid = qam_grid(a.n_wg), block(QAM_THREADS);
    const bool csi = a.csi_period > 0, perm = a.perm != nullptr;
    if (csi && perm) hipLaunchKernelGGL((qam_demap_kernel<BPS, true, true>), grid, block, 0, st, a);
    else if (csi) hipLaunchKernelGGL((qam_demap_kernel<BPS, true, false>), grid, block, 0, st, a);
    else if (perm) hipLaunchKernelGGL((qam_demap_kernel<BPS, false, true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((qam_demap_kernel<BPS, false, false>), grid, block, 0, st, a);
    SFE_HIP(hipGetLastError());
    return SFE_OK;
}

template <int BPS>
int qam_map_go(const QamArgs &a, hipStream_t st)
{
    const dim3 grid = qam_grid(a.n_wg), block(QAM_THREADS);
    if (a.perm) hipLaunchKernelGGL((qam_map_kernel<BPS, true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((qam_map_kernel<BPS, false>), grid, block, 0, st, a);
    SFE_HIP(hipGetLastError());
    return SFE_OK;
}

}  // namespace

int launch_qam_demap(int bps, const QamArgs &a, hipStream_t st)
{
    if (a.n_wg == 0) return SFE_OK;
    switch (bps) {
    case 1: return qam_demap_go<1>(a, st);
    case 2: return qam_demap_go<2>(a, st);
    case 4: return qam_demap_go<4>(a, st);
    case 6: return qam_demap_go<6>(a, st);
    case 8: return qam_demap_go<8>(a, st);
    }
    set_error("qam: %d bits per symbol have no kernel", bps);
    return SFE_EINVAL;
}

int launch_qam_map(int bps, const QamArgs &a, hipStream_t st)
{
    if (a.n_wg == 0) return SFE_OK;
    switch (bps) {
    case 1: return qam_map_go<1>(a, st);
    case 2: return qam_map_go<2>(a, st);
    case 4: return qam_map_go<4>(a, st);
    case 6: return qam_map_go<6>(a, st);
    case 8: return qam_map_go<8>(a, st);
    }
    set_error("qam: %d bits per symbol have no kernel", bps);
    return SFE_EINVAL;
}

}  // namespace sfe
