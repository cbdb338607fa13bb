// iir.hip -- streaming biquad-cascade IIR filter (sfe_dsp_iir_*): S second-order sections over every stream.
//
//   v_0 = x,   v_{s+1}[i] = b0_s v_s[i] + b1_s v_s[i-1] + b2_s v_s[i-2] - a1_s v_{s+1}[i-1] - a2_s v_{s+1}[i-2],   y = v_S
//
// A linear recurrence over one long stream, parallelised exactly by block decomposition.  A section in transposed direct
// form II carries a 2-vector s:  y = b0 x + s.x;  s' = A s + B x  with  A = [[-a1, 1], [-a2, 0]].  Over a span of m
// samples the output is the zero-state response plus [1 0] A^k s_start, and the end state is A^m s_start plus the
// zero-state end state.  Everything below is that identity applied at three scales, every product-sum an explicit fmaf
// in a fixed order (the file is compiled with -ffp-contract=off), I and Q never mixed: a complex stream is two
// components that run the arithmetic of a real stream each.
//
// A block is G = 4096 samples of one stream: one workgroup of 256 threads, thread t owning the run [16 t, 16 t + 16).
//   iir_block_kernel, per section in cascade order:
//     1. the recursion over the run from zero state, in registers: the outputs and the run's zero-state end state z_t;
//     2. the scan s_{t+1} = A^16 s_t + z_t over the workgroup: Kogge-Stone over the 64 lanes of a wave with the host's
//        float32 A^(16 2^k), the four wave totals through LDS, the wave start states by a sequential fold with A^1024,
//        s_t = (exclusive wave scan) + A^(16 lane) (wave start state);
//     3. the correction y[k] += [1 0] A^k s_t from a table; the next section reads the corrected values.
//   Samples come in and go out coalesced, through an LDS image whose runs are 17 floats apart (conflict-free both ways).
// Across blocks, three launches on the caller's stream:
//   pass 1  iir_block_kernel<.., false>: every block from zero state; its end state z_b (2S floats per component) into
//           the handle's table;
//   fold    the true state T(b) at the start of every block, from T(b + 1) = Phi T(b) + z_b (Phi: the cascade's 2S x 2S
//           transition over G samples, float64 on the host, rounded once).  A chain of n / G dependent steps would cost
//           more than both passes (65 536 steps for 2^28 samples), so it has two levels on ABSOLUTE block indices (counted
//           by the host since create / reset): a group is K = 128 consecutive blocks, and with Z_g the zero-state fold
//           of the group's z_b,
//               T(gK) = S_g,   S_0 = 0,   S_{g+1} = Phi^K S_g + Z_g;        T(gK + j + 1) = Phi T(gK + j) + z_{gK+j}
//           iir_group_kernel<false> folds every group's Z_g (one wave per group and chain), iir_chain_kernel walks the
//           S_g (one wave per chain), iir_group_kernel<true> walks every group's T(b), overwriting z_b.  The carried state
//           is T, S_g and the partial fold of the open group, so a call that begins or ends inside a group continues
//           the same sums: the grouping never depends on where calls are cut;
//   pass 3  iir_block_kernel<.., true>: every block from its start state, storing the output.
// Every value is a function of the samples and of absolute position alone, so any cut of the stream at a multiple of G
// gives the same bits, and nothing depends on which workgroup finishes first.
#include "iir.h"

namespace sfe {

namespace {

constexpr int IIR_THREADS = 256;
constexpr int IIR_R = 16;                       // samples per thread
constexpr int IIR_G = IIR_THREADS * IIR_R;      // samples per block
constexpr int IIR_PITCH = IIR_R + 1;            // floats between two runs in LDS
constexpr int IIR_PLANE = IIR_THREADS * IIR_PITCH;
constexpr int IIR_WAVES = IIR_THREADS / 64;
constexpr int IIR_K = 128;                      // blocks per group of the fold
constexpr int IIR_AHEAD = 8;                    // table entries a fold kernel loads ahead of its dependent steps

enum { IIR_CF32 = 0, IIR_U8 = 1, IIR_REAL = 2 };

// One section's float32 constants, as the host lays them out (api_iir.hip: IIR_SEC_FLOATS each)
struct IirSec {
    float b0, b1, b2, a1, a2, pad[3];
    float M[7][4];              // A^(16 2^k), k = 0..6, row-major (k = 6: a whole wave)
    float c[IIR_R][2];          // [1 0] A^k
    float P[64][4];             // A^(16 l), l = 0..63
};
static_assert(sizeof(IirSec) == 4 * IIR_SEC_FLOATS, "the host's layout");

struct IirArgs {
    const void *in;
    void *out;
    const IirSec *sec;          // [S]
    const float *phi, *phik;    // [2S][2S] row-major: the cascade's transition over G and over K G samples
    float *table;               // [n_streams][nb][NC][2S]: pass 1's end states, then the fold's start states
    float *gtable;              // [n_streams][ng][NC][2S]: the groups' zero-state folds, then their start states
    const float *state_cur;     // [n_streams][NC][3][2S]: carried (struct IirSpan)
    float *state_nxt;
    long long in_stride, out_stride;
    long long B0;               // absolute index of the call's first block
    int nb, ng, K, S;
};

struct f2 {
    float x, y;
};

// M v + w, M row-major 2x2
__device__ __forceinline__ f2 iir_mv(const float *M, f2 v, f2 w)
{
    return f2{fmaf(M[0], v.x, fmaf(M[1], v.y, w.x)), fmaf(M[2], v.x, fmaf(M[3], v.y, w.y))};
}

template <int FMT, bool FINAL>
__global__ __launch_bounds__(IIR_THREADS) void iir_block_kernel(IirArgs a)
{
    constexpr int NC = FMT == IIR_REAL ? 1 : 2;
    __shared__ float V[NC * IIR_PLANE];
    __shared__ float W[IIR_MAX_SECTIONS][IIR_WAVES][NC][2];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long b = blockIdx.x, s = blockIdx.y;
    const long long base = b * IIR_G;
    const int S = a.S;

    // fetch: element i = e 256 + tid of the block, contiguous across lanes, to its place in the padded image
#pragma unroll
    for (int e = 0; e < IIR_R; e++) {
        const int i = e * IIR_THREADS + tid, at = i + (i >> 4);
        if constexpr (FMT == IIR_CF32) {
            const v2f x = static_cast<const v2f *>(a.in)[s * a.in_stride + base + i];
            V[at] = x.x;
            V[IIR_PLANE + at] = x.y;
        } else if constexpr (FMT == IIR_U8) {
            const unsigned w = static_cast<const unsigned short *>(a.in)[s * a.in_stride + base + i];
            V[at] = u8_to_f32(w & 0xffu);
            V[IIR_PLANE + at] = u8_to_f32(w >> 8);
        } else {
            V[at] = static_cast<const float *>(a.in)[s * a.in_stride + base + i];
        }
    }
    lds_barrier();
    float v[NC][IIR_R];
#pragma unroll
    for (int c = 0; c < NC; c++)
#pragma unroll
        for (int k = 0; k < IIR_R; k++) v[c][k] = V[c * IIR_PLANE + tid * IIR_PITCH + k];

    const float *start = a.table + ((s * a.nb + b) * NC) * 2 * S;       // FINAL: this block's start state
    float *zend = a.table + ((s * a.nb + b) * NC) * 2 * S;              // else: its zero-state end state goes here

    for (int q = 0; q < S; q++) {
        const IirSec &h = a.sec[q];
        const float b0 = h.b0, b1 = h.b1, b2 = h.b2, na1 = -h.a1, na2 = -h.a2;
        f2 acc[NC];
        // 1. the run from zero state
#pragma unroll
        for (int c = 0; c < NC; c++) {
            float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
            for (int k = 0; k < IIR_R; k++) {
                const float x = v[c][k];
                const float y = fmaf(b0, x, s1);
                s1 = fmaf(na1, y, fmaf(b1, x, s2));
                s2 = fmaf(na2, y, b2 * x);
                v[c][k] = y;
            }
            acc[c] = f2{s1, s2};
        }
        // 2. inclusive scan over the wave: after step k, acc covers the 2^(k+1) runs that end with this lane's
#pragma unroll
        for (int k = 0; k < 6; k++) {
#pragma unroll
            for (int c = 0; c < NC; c++) {
                const f2 u{__shfl_up(acc[c].x, 1u << k, 64), __shfl_up(acc[c].y, 1u << k, 64)};
                if (lane >= (1 << k)) acc[c] = iir_mv(h.M[k], u, acc[c]);
            }
        }
        if (lane == 63) {
#pragma unroll
            for (int c = 0; c < NC; c++) {
                W[q][wave][c][0] = acc[c].x;
                W[q][wave][c][1] = acc[c].y;
            }
        }
        lds_barrier();
#pragma unroll
        for (int c = 0; c < NC; c++) {
            // the wave's start state: the block's, folded over the waves before this one
            f2 sg{0.0f, 0.0f};
            if constexpr (FINAL) sg = f2{start[c * 2 * S + 2 * q], start[c * 2 * S + 2 * q + 1]};
            for (int w = 0; w < wave; w++) sg = iir_mv(h.M[6], sg, f2{W[q][w][c][0], W[q][w][c][1]});
            if constexpr (!FINAL) {
                if (tid == IIR_THREADS - 1) {
                    const f2 e = iir_mv(h.M[6], sg, acc[c]);
                    zend[c * 2 * S + 2 * q] = e.x;
                    zend[c * 2 * S + 2 * q + 1] = e.y;
                }
                if (q == S - 1) continue;           // the last section's outputs are not needed for the end state
            }
            // this run's start state, then 3. the correction
            f2 ex{__shfl_up(acc[c].x, 1u, 64), __shfl_up(acc[c].y, 1u, 64)};
            if (lane == 0) ex = f2{0.0f, 0.0f};
            const f2 st = iir_mv(h.P[lane], sg, ex);
#pragma unroll
            for (int k = 0; k < IIR_R; k++) v[c][k] = fmaf(h.c[k][0], st.x, fmaf(h.c[k][1], st.y, v[c][k]));
        }
    }

    if constexpr (FINAL) {
#pragma unroll
        for (int c = 0; c < NC; c++)
#pragma unroll
            for (int k = 0; k < IIR_R; k++) V[c * IIR_PLANE + tid * IIR_PITCH + k] = v[c][k];
        lds_barrier();
#pragma unroll
        for (int e = 0; e < IIR_R; e++) {
            const int i = e * IIR_THREADS + tid, at = i + (i >> 4);
            if constexpr (NC == 2) static_cast<v2f *>(a.out)[s * a.out_stride + base + i] = v2f{V[at], V[IIR_PLANE + at]};
            else static_cast<float *>(a.out)[s * a.out_stride + base + i] = V[at];
        }
    }
}

// ---- the fold over the blocks' states.  One wave per chain (a stream's component): lane j < 2S holds row j of the matrix and
// element j of the state; a step is st' = M st + z, the columns taken in two ascending interleaved sums.
struct IirRow {
    float m[2 * IIR_MAX_SECTIONS];
};

__device__ __forceinline__ IirRow iir_row(const float *M, int n, int j)
{
    IirRow r;
#pragma unroll
    for (int k = 0; k < 2 * IIR_MAX_SECTIONS; k++) r.m[k] = k < n ? M[j * n + k] : 0.0f;
    return r;
}

__device__ __forceinline__ float iir_step(const IirRow &r, float st, float z, int n)
{
    float e = z, o = 0.0f;
#pragma unroll
    for (int k = 0; k < 2 * IIR_MAX_SECTIONS; k += 2) {
        if (k < n) {                        // n is even and the same for every lane
            e = fmaf(r.m[k], __int_as_float(__builtin_amdgcn_readlane(__float_as_int(st), k)), e);
            o = fmaf(r.m[k + 1], __int_as_float(__builtin_amdgcn_readlane(__float_as_int(st), k + 1)), o);
        }
    }
    return e + o;
}

// The blocks of one group (K consecutive blocks, counted from create / reset) that lie inside the call, for one chain.
struct IirSpan {
    long long g, lo, hi;        // absolute group; absolute blocks [lo, hi)
    bool opens, closes, last;   // the call holds the group's first block / its last block; the call's last group
    float *slot, *gslot;        // the first block's entry of the table; the group's entry of the group table (lane j's element)
    const float *cur;           // carried state of the chain: [3][2S] = the true state T, the open group's zero-state fold Zp,
    float *nxt;                 // the open group's start state Sg; read from cur, written to nxt (the host swaps them)
    long long pitch;
};

__device__ __forceinline__ IirSpan iir_span(const IirArgs &a, int NC, int g_rel, int chain, int j)
{
    const int n = 2 * a.S;
    const long long s = chain / NC, c = chain % NC;
    IirSpan p;
    p.g = a.B0 / a.K + g_rel;
    p.lo = p.g * a.K > a.B0 ? p.g * a.K : a.B0;
    p.hi = (p.g + 1) * a.K < a.B0 + a.nb ? (p.g + 1) * a.K : a.B0 + a.nb;
    p.opens = p.lo == p.g * a.K;
    p.closes = p.hi == (p.g + 1) * a.K;
    p.last = g_rel == a.ng - 1;
    p.pitch = (long long)NC * n;
    p.slot = a.table + ((s * a.nb + (p.lo - a.B0)) * NC + c) * n + j;
    p.gslot = a.gtable + ((s * a.ng + g_rel) * NC + c) * n + j;
    p.cur = a.state_cur + (long long)chain * 3 * n;
    p.nxt = a.state_nxt + (long long)chain * 3 * n;
    return p;
}

// Level 1 (CHAIN = false): every group's zero-state fold Z_g over its blocks' end states z_b, ascending; the group that was
// open when the call began continues from the carried partial fold.  A group that closes leaves Z_g in the group table,
// the one that stays open leaves its partial fold in the carried state.
// Level 3 (CHAIN = true): every group's chain T(b + 1) = Phi T(b) + z_b from the group's start state (the group table,
// written by level 2), or from the carried true state for the group that was open; z_b is overwritten by T(b).
template <bool CHAIN>
__global__ __launch_bounds__(64) void iir_group_kernel(IirArgs a, int NC)
{
    const int n = 2 * a.S, j = threadIdx.x < n ? threadIdx.x : 0;
    const bool own = threadIdx.x < n;
    const IirSpan p = iir_span(a, NC, blockIdx.x, blockIdx.y, j);
    const IirRow phi = iir_row(a.phi, n, j);
    float st;
    if constexpr (CHAIN) st = p.opens ? p.gslot[0] : p.cur[j];
    else st = p.opens ? 0.0f : p.cur[n + j];
    float *slot = p.slot;
    for (long long b0 = p.lo; b0 < p.hi; b0 += IIR_AHEAD) {           // IIR_AHEAD blocks' z_b in flight over their steps
        float z[IIR_AHEAD];
#pragma unroll
        for (int i = 0; i < IIR_AHEAD; i++) z[i] = b0 + i < p.hi ? slot[i * p.pitch] : 0.0f;
#pragma unroll
        for (int i = 0; i < IIR_AHEAD; i++) {
            if (b0 + i < p.hi) {
                if (CHAIN && own) slot[i * p.pitch] = st;
                st = iir_step(phi, st, z[i], n);
            }
        }
        slot += IIR_AHEAD * p.pitch;
    }
    if (!own) return;
    if constexpr (CHAIN) {
        // the state the next call starts from: a group's start state where the call ends on a group boundary
        if (p.last) p.nxt[j] = p.closes ? p.nxt[2 * n + j] : st;
    } else {
        if (p.closes) p.gslot[0] = st;
        if (p.last) p.nxt[n + j] = p.closes ? 0.0f : st;
    }
}

// Level 2: the groups' start states S_{g+1} = Phi^K S_g + Z_g, ascending from the carried one; Z_g is overwritten by S_g.
__global__ __launch_bounds__(64) void iir_chain_kernel(IirArgs a, int NC)
{
    const int n = 2 * a.S, j = threadIdx.x < n ? threadIdx.x : 0;
    const bool own = threadIdx.x < n;
    const IirSpan p = iir_span(a, NC, 0, blockIdx.x, j);
    const IirRow phik = iir_row(a.phik, n, j);
    const long long end = a.B0 + a.nb;
    float st = p.cur[2 * n + j];
    float *gs = p.gslot;
    const int closing = (int)(end / a.K - p.g);                     // the call's groups that close: all of them, or all but the last
    for (int g0 = 0; g0 < a.ng; g0 += IIR_AHEAD) {
        float z[IIR_AHEAD];
#pragma unroll
        for (int i = 0; i < IIR_AHEAD; i++) z[i] = g0 + i < closing ? gs[i * p.pitch] : 0.0f;
#pragma unroll
        for (int i = 0; i < IIR_AHEAD; i++) {
            if (g0 + i < a.ng) {
                if (own) gs[i * p.pitch] = st;
                if (g0 + i < closing) st = iir_step(phik, st, z[i], n);
            }
        }
        gs += IIR_AHEAD * p.pitch;
    }
    if (own) p.nxt[2 * n + j] = st;
}

template <int FMT>
int iir_launch_fmt(const IirArgs &a, int n_streams, hipStream_t st)
{
    const dim3 grid((unsigned)a.nb, (unsigned)n_streams);
    constexpr int NC = FMT == IIR_REAL ? 1 : 2;
    const dim3 ggrid((unsigned)a.ng, (unsigned)(n_streams * NC));
    hipLaunchKernelGGL((iir_block_kernel<FMT, false>), grid, dim3(IIR_THREADS), 0, st, a);
    SFE_HIP(hipGetLastError());
    hipLaunchKernelGGL(iir_group_kernel<false>, ggrid, dim3(64), 0, st, a, NC);
    SFE_HIP(hipGetLastError());
    hipLaunchKernelGGL(iir_chain_kernel, dim3((unsigned)(n_streams * NC)), dim3(64), 0, st, a, NC);
    SFE_HIP(hipGetLastError());
    hipLaunchKernelGGL(iir_group_kernel<true>, ggrid, dim3(64), 0, st, a, NC);
    SFE_HIP(hipGetLastError());
    hipLaunchKernelGGL((iir_block_kernel<FMT, true>), grid, dim3(IIR_THREADS), 0, st, a);
    SFE_HIP(hipGetLastError());
    return SFE_OK;
}

}  // namespace

int iir_block() { return IIR_G; }
int iir_group() { return IIR_K; }

// The groups a call of nb blocks touches when it starts at absolute block B0
int iir_groups(long long B0, int nb) { return (int)((B0 + nb - 1) / IIR_K - B0 / IIR_K + 1); }

// One call: nb = n_in / G blocks of every stream, the first of them absolute block B0 since create / reset.  Shapes and
// buffers are the caller's (api_iir.hip) to check: 1 <= S <= 8, nb >= 1, a table of n_streams (nb + iir_groups()) NC 2S
// floats, carried state of n_streams NC 3 2S floats twice, n_streams NC <= 65535.  fmt: 0 cf32, 1 u8 pairs, 2 real float32.
int launch_iir(int fmt, const void *in, long long in_stride, void *out, long long out_stride, const void *sec, const float *phi,
               const float *phik, float *table, const float *state_cur, float *state_nxt, long long B0, int nb, int S, int n_streams,
               hipStream_t st)
{
    const int ng = iir_groups(B0, nb), NC = fmt == IIR_REAL ? 1 : 2;
    IirArgs a{in, out, static_cast<const IirSec *>(sec), phi, phik, table, table + (long long)n_streams * nb * NC * 2 * S, state_cur,
              state_nxt, in_stride, out_stride, B0, nb, ng, IIR_K, S};
    switch (fmt) {
    case IIR_CF32: return iir_launch_fmt<IIR_CF32>(a, n_streams, st);
    case IIR_U8: return iir_launch_fmt<IIR_U8>(a, n_streams, st);
    case IIR_REAL: return iir_launch_fmt<IIR_REAL>(a, n_streams, st);
    }
    set_error("iir: format %d has no kernel", fmt);
    return SFE_EINVAL;
}

}  // namespace sfe
