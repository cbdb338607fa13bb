// cov.hip -- streaming spatial covariance estimator (sfe_dsp_cov_*): the sample covariance of S streams, per band.
//
//   u[2s] = Re x_{s,k}[m],  u[2s+1] = Im x_{s,k}[m]                     instant m of band k as a real column of 2S floats
//   G_r[i][j] = scale * sum over m in [rA, (r + 1)A) of u_i[m] u_j[m]    2S x 2S float32, row-major, both triangles
//
// The order of that sum is part of the contract (include/sfe_dsp.h): a row's instants go in chunks of T = COV_T
// consecutive instants, the chunks in groups of C consecutive chunks (C the smallest power of two with C C >= A / T),
// all counted from the row's first.  A chunk partial is the float32 fmaf chain from +0 over its T products, ascending;
// a group sum the float32 left fold, from 0, of its chunk partials; the row the left fold, from 0, of its group sums.
//
// v_mfma_f32_16x16x4_f32 with K = four consecutive instants: D[16 x 16] += A[16 x 4] B[4 x 16], A = row tile I of U at
// instants 4q .. 4q+3, B = row tile J of U at the same instants, transposed.  Lane l = 16 kq + i hands the pipe
// u_{16I+i}[4q + kq] and u_{16J+i}[4q + kq]; sixteen such instructions in a row on one accumulator that starts at zero
// ARE the chunk partial of 256 entries, bit for bit.  Only the tiles I <= J are computed (36 of 64 at S = 64); the
// final store mirrors them, so G[i][j] and G[j][i] are one float written twice.
//
// Operand fetch: a chunk of U is staged in LDS as [row][instant], pitch T + 4 floats.  Writing it, a wave takes one
// stream and its 64 lanes the 64 instants: one 8-byte load per lane (512 contiguous bytes of a stream; u8: 128), two
// LDS stores of consecutive words.  Reading it, lane (kq, i) takes word (16I + i) pitch + 4q + kq: with the pitch
// 4 mod 64 the 64 lanes of a read fall in 64 different banks.  Rows 2S .. 16 NT - 1 (the padding of the last tile) are
// zeroed once and never loaded: they are zero on both sides of every product, so a NaN cannot leak through 0 x NaN.
// The next chunk's global loads are issued before this chunk's products.
//
// The host (api_cov.hip) counts chunks; a call that starts j0 chunks into a row and completes q of them is laid out in
// row-relative chunk indices [j0, j0 + q), group g' = r' GPR + c (GPR groups per row) being the chunks [r' AC + c C,
// min(.. + C, (r' + 1) AC)), AC = A / T.  Two launches:
//   1. cov_chunk_kernel: one workgroup per band and group piece (the part of one group inside the call).  Its waves
//      (1, 3 or 4: as many as there are tiles, four at the most) share the staged chunk and own every WAVES-th tile:
//      two accumulator sets per tile, the chunk partial from zero and `group += partial`.  The group sum starts from
//      the carried open-group value when the piece starts mid-group and goes to the other buffer of that pair when the
//      piece ends mid-group, else to the call's scratch of group sums -- all in fragment order (cov.h).
//   2. cov_row_kernel: one lane per (band, row touched, tile, fragment lane) folds the row's group sums that this call
//      completed, starting from the carried open-row value when the row began in an earlier call; a row that completes
//      goes out times scale, mirrored; one that stays open goes to the other buffer of the open-row pair.  With one
//      chunk per row (A = T) the row is 0 + (0 + partial): the chunk kernel writes it itself, no scratch, no row kernel.
// No atomics, and nothing depends on the order in which workgroups run.
#include "cov.h"

namespace sfe {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int COV_PITCH = COV_T + 4;    // floats per staged row: 4 mod 64

struct CovArgs {
    const void *in;             // call input: x_{s,k} at in + (s M + k) in_stride samples (cf32, or u8 (I,Q) pairs)
    const float *group_in;      // [M][FR]: the open group's fold so far, FR = cov_frag_floats(S)
    float *group_out;
    const float *row_in;        // [M][FR]: the open row's fold so far
    float *row_out;
    float *scratch;             // [M][pieces][FR]: the group sums this call completes (unused when GPR = 1)
    float *out;
    long long in_stride, out_stride;
    long long j0, end;          // the call's chunks, row-relative: [j0, end), j0 < AC
    int S, M, AC, C, GPR, c0;   // c0 = j0 / C: the group of piece 0
    int pieces, rows;           // rows touched: (end - 1) / AC + 1
    float scale;
};

__host__ __device__ __forceinline__ long long cov_min(long long x, long long y) { return x < y ? x : y; }
__host__ __device__ __forceinline__ long long cov_max(long long x, long long y) { return x > y ? x : y; }

constexpr int cov_waves(int NT) { return NT == 1 ? 1 : NT == 2 ? 3 : 4; }

// tile t of an NT-tile triangle is (I, J), I <= J
__device__ __forceinline__ void cov_tile_ij(int NT, int t, int &I, int &J)
{
    I = 0;
    while (t >= NT - I) {
        t -= NT - I;
        I++;
    }
    J = I + t;
}

// the entries of tile (I, J) this lane holds, into a 2S x 2S row-major matrix: the upper triangle and its mirror
__device__ __forceinline__ void cov_store_tile(float *G, int n2, int I, int J, unsigned lane, f32x4 v)
{
    const int col = 16 * J + (int)(lane & 15), row0 = 16 * I + 4 * (int)(lane >> 4);
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int row = row0 + r;
        if (col < n2 && row <= col) {
            G[(size_t)row * n2 + col] = v[r];
            if (row != col) G[(size_t)col * n2 + row] = v[r];
        }
    }
}

template <int NT, bool U8>
__global__ __launch_bounds__(64 * cov_waves(NT)) void cov_chunk_kernel(CovArgs a)
{
    constexpr int WAVES = cov_waves(NT), THREADS = 64 * WAVES, NTILES = NT * (NT + 1) / 2;
    constexpr int TPW = (NTILES + WAVES - 1) / WAVES;           // tiles per wave
    constexpr int SPW = (8 * NT + WAVES - 1) / WAVES;           // streams a wave stages, at the most
    constexpr int FR = NTILES * 256;
    __shared__ float U[16 * NT * COV_PITCH];

    const unsigned tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const size_t band = blockIdx.y;
    const int p = blockIdx.x, S = a.S;

    // the group of this piece, and the part of it inside the call (row-relative chunk indices)
    const long long g = (long long)a.c0 + p;
    const int r = (int)(g / a.GPR), c = (int)(g % a.GPR);
    const long long cs = (long long)r * a.AC + (long long)c * a.C;
    const long long ce = cov_min(cs + a.C, (long long)(r + 1) * a.AC);
    const long long lo = cov_max(cs, a.j0), hi = cov_min(ce, a.end);

    // padding rows: zero, for good
    for (unsigned i = 2 * S * COV_PITCH + tid; i < 16u * NT * COV_PITCH; i += THREADS) U[i] = 0.0f;

    // this wave's tiles; one past the last is computed as tile 0 again and not stored
    int offA[TPW], offB[TPW];
    f32x4 grp[TPW];
#pragma unroll
    for (int e = 0; e < TPW; e++) {
        const int t = wave + e * WAVES;
        int I, J;
        cov_tile_ij(NT, t < NTILES ? t : 0, I, J);
        offA[e] = (16 * I + (int)(lane & 15)) * COV_PITCH + (int)(lane >> 4);
        offB[e] = (16 * J + (int)(lane & 15)) * COV_PITCH + (int)(lane >> 4);
        grp[e] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        if (lo > cs && t < NTILES) grp[e] = reinterpret_cast<const f32x4 *>(a.group_in + band * FR)[t * 64 + lane];
    }

    // chunk t (row-relative) of this wave's streams, WAVES apart: this lane's instant.  One address, stepped.
    // The masks "e < ns" are the same for every chunk: recomputed per chunk (a scalar compare each) instead of kept,
    // 2 SPW wave masks in scalar registers, across the loop.
    const size_t step = (size_t)WAVES * a.M * (size_t)a.in_stride;
    const int ns0 = S > wave ? (S - wave + WAVES - 1) / WAVES : 0;      // streams this wave stages
    auto fetch = [&](long long t, v2f (&x)[SPW]) {
        int ns = ns0;
        asm volatile("" : "+s"(ns));
        size_t at = ((size_t)wave * a.M + band) * (size_t)a.in_stride + (size_t)(t - a.j0) * COV_T + lane;
#pragma unroll
        for (int e = 0; e < SPW; e++) {
            x[e] = v2f{0.0f, 0.0f};
            if (e < ns) {
                if constexpr (U8) {
                    const unsigned w = __builtin_nontemporal_load(static_cast<const unsigned short *>(a.in) + at);
                    x[e] = v2f{u8_to_f32(w & 0xffu), u8_to_f32(w >> 8)};
                } else {
                    x[e] = __builtin_nontemporal_load(static_cast<const v2f *>(a.in) + at);
                }
            }
            at += step;
        }
    };

    v2f x[SPW];
    fetch(lo, x);
    for (long long t = lo; t < hi; t++) {
        int ns = ns0;
        asm volatile("" : "+s"(ns));
#pragma unroll
        for (int e = 0; e < SPW; e++) {
            const int s = wave + e * WAVES;
            if (e < ns) {
                U[(2 * s) * COV_PITCH + lane] = x[e].x;
                U[(2 * s + 1) * COV_PITCH + lane] = x[e].y;
            }
        }
        if (t + 1 < hi) fetch(t + 1, x);            // in flight over the products
        lds_barrier();

        f32x4 part[TPW];
#pragma unroll
        for (int e = 0; e < TPW; e++) part[e] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int q = 0; q < COV_T / 4; q++) {
#pragma unroll
            for (int e = 0; e < TPW; e++)
                part[e] = __builtin_amdgcn_mfma_f32_16x16x4f32(U[offA[e] + 4 * q], U[offB[e] + 4 * q], part[e], 0, 0, 0);
        }
#pragma unroll
        for (int e = 0; e < TPW; e++) grp[e] = grp[e] + part[e];
        lds_barrier();
    }

    if (hi == ce && a.GPR == 1) {
        // a chunk that is a whole row (A = T): the row is 0 + its one group sum, so it goes straight out
        float *G = a.out + band * (size_t)a.out_stride + (size_t)r * (4 * S * S);
#pragma unroll
        for (int e = 0; e < TPW; e++) {
            const int t = wave + e * WAVES;
            if (t >= NTILES) break;
            int I, J;
            cov_tile_ij(NT, t, I, J);
            cov_store_tile(G, 2 * S, I, J, lane, a.scale * (f32x4{0.0f, 0.0f, 0.0f, 0.0f} + grp[e]));
        }
        return;
    }
    float *dst = hi < ce ? a.group_out + band * FR : a.scratch + (band * a.pieces + p) * FR;
#pragma unroll
    for (int e = 0; e < TPW; e++)
        if (wave + e * WAVES < NTILES) reinterpret_cast<f32x4 *>(dst)[(wave + e * WAVES) * 64 + lane] = grp[e];
}

// blockIdx.x = row touched * TB + block of four tiles, blockIdx.y = band; one wave per tile
__global__ __launch_bounds__(256) void cov_row_kernel(CovArgs a, int NT, int TB)
{
    const int NTILES = NT * (NT + 1) / 2, FR4 = NTILES * 64;
    const unsigned lane = threadIdx.x & 63;
    const int tile = (int)(blockIdx.x % TB) * 4 + (int)(threadIdx.x >> 6), r = (int)(blockIdx.x / TB);
    const size_t band = blockIdx.y;
    if (tile >= NTILES) return;
    const long long row_lo = (long long)r * a.AC, row_hi = row_lo + a.AC;
    const size_t at = (size_t)tile * 64 + lane;

    f32x4 sum = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    if (r == 0 && a.j0 > 0) sum = reinterpret_cast<const f32x4 *>(a.row_in)[band * FR4 + at];
    const long long p0 = (long long)band * a.pieces + (long long)r * a.GPR - a.c0;      // piece of the row's group 0
    const f32x4 *sc = reinterpret_cast<const f32x4 *>(a.scratch);
    for (int c = r == 0 ? a.c0 : 0; c < a.GPR; c++) {
        if (cov_min(row_lo + (long long)(c + 1) * a.C, row_hi) > a.end) break;      // still open when the call ends
        sum = sum + sc[(size_t)(p0 + c) * FR4 + at];
    }
    if (row_hi <= a.end) {
        int I, J;
        cov_tile_ij(NT, tile, I, J);
        cov_store_tile(a.out + band * (size_t)a.out_stride + (size_t)r * (4 * a.S * a.S), 2 * a.S, I, J, lane, a.scale * sum);
    } else {
        reinterpret_cast<f32x4 *>(a.row_out)[band * FR4 + at] = sum;
    }
}

template <int NT, bool U8>
int cov_launch(const CovArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL((cov_chunk_kernel<NT, U8>), dim3((unsigned)a.pieces, (unsigned)a.M), dim3(64 * cov_waves(NT)), 0, st, a);
    SFE_HIP(hipGetLastError());
    if (a.GPR > 1) {                        // with one chunk per row the chunk kernel has written the rows itself
        const int TB = (NT * (NT + 1) / 2 + 3) / 4;
        hipLaunchKernelGGL(cov_row_kernel, dim3((unsigned)((long long)a.rows * TB), (unsigned)a.M), dim3(256), 0, st, a, NT, TB);
        SFE_HIP(hipGetLastError());
    }
    return SFE_OK;
}

template <bool U8>
int cov_launch_nt(int NT, const CovArgs &a, hipStream_t st)
{
    switch (NT) {
    case 1: return cov_launch<1, U8>(a, st);
    case 2: return cov_launch<2, U8>(a, st);
    case 3: return cov_launch<3, U8>(a, st);
    case 4: return cov_launch<4, U8>(a, st);
    case 5: return cov_launch<5, U8>(a, st);
    case 6: return cov_launch<6, U8>(a, st);
    case 7: return cov_launch<7, U8>(a, st);
    case 8: return cov_launch<8, U8>(a, st);
    }
    set_error("cov: no kernel for %d row tiles", NT);
    return SFE_EINVAL;
}

}  // namespace

long long cov_pieces(long long j0, long long q, int AC, int C, long long *rows)
{
    const long long GPR = (AC + C - 1) / C, last = j0 + q - 1;
    if (rows) *rows = last / AC + 1;
    return (last / AC) * GPR + (last % AC) / C - j0 / C + 1;
}

int launch_cov(int u8, const void *in, long long in_stride, const float *group_in, float *group_out, const float *row_in,
               float *row_out, float *scratch, float *out, long long out_stride, long long n_in, int S, int M, int AC, int C,
               long long j0, float scale, hipStream_t st)
{
    const long long q = n_in / COV_T;
    long long rows = 0;
    const long long pieces = cov_pieces(j0, q, AC, C, &rows);
    const int NT = cov_nt(S);
    if (pieces > 0x7fffffffLL || rows * ((NT * (NT + 1) / 2 + 3) / 4) > 0x7fffffffLL) {
        set_error("cov_process_stream: call too large for one grid");
        return SFE_EINVAL;
    }
    const CovArgs a{in, group_in, group_out, row_in, row_out, scratch, out, in_stride, out_stride, j0, j0 + q,
                    S, M, AC, C, (AC + C - 1) / C, (int)(j0 / C), (int)pieces, (int)rows, scale};
    return u8 ? cov_launch_nt<true>(NT, a, st) : cov_launch_nt<false>(NT, a, st);
}

}  // namespace sfe
