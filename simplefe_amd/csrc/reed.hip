// reed.hip -- the kernels of the Reed-Solomon outer code (sfe_dsp_reed_*, include/sfe_dsp.h): interleaved frames to payloads
// (decode) and payloads to frames (encode), by the law of reed_law.h.  Integer work only; the host plan (api_reed.hip) states
// the same law serially, and the two give the same bytes because the law determines them.
//
// One launch, 256 threads: a workgroup holds 16 codewords in LDS -- one frame of depth >= 4, or 4 / depth frames below that --
// and each of its four waves takes a codeword at a time.
//   - a frame's bytes are read once, in aligned dwords with bytes at the ragged ends whatever the address is, de-whitened
//     against a copy of the sequence shifted to the same alignment, and scattered byte by byte into the codewords' rows;
//   - a wave keeps its codeword's 256-byte row in one register (lane l the dword l), so the byte of a step is a lane read
//     with a uniform index into a scalar: the loops over a codeword's bytes wait for no LDS access;
//   - syndromes: lane i < n_par runs Horner with its own root.  The multiply by the lane's constant is the shift-and-xor
//     multiply with the constant's eight products root x^b kept in registers: eight (bit-extract, and, xor);
//   - a ballot of zero syndromes ends a clean codeword there;
//   - otherwise the inversion-free Berlekamp-Massey recurrence, Lambda and x^m B a coefficient a lane: the discrepancy is
//     eight ballots' parities (a scalar), the update two multiplies by a scalar; n_par steps whatever the data is;
//   - the root search takes 64 positions at a time, a lane a position (four rounds at n = 255), Horner over the t + 1
//     coefficients read lane by lane; ballots count the roots; Forney's magnitudes for the rounds that hold a root;
//   - only a codeword with L <= t, degree L and L roots among its n positions is patched, in LDS;
//   - encode: n_par lanes hold the remainder register, the feedback byte is a scalar.
// Every trip count is a function of (n, n_par) alone.  No scratch, no global atomics; the per-frame sums are integer LDS
// atomics, so no order shows in them.
#include "reed.h"

namespace sfe {
namespace {

constexpr int T = 64 * REED_WAVES;

__device__ __forceinline__ unsigned xtime(unsigned a, unsigned prim)
{
    a <<= 1;
    return a ^ ((0u - ((a >> 8) & 1u)) & prim);
}

// s times the constant whose products with x^b are c[b]
__device__ __forceinline__ unsigned mul_const(const unsigned (&c)[8], unsigned s)
{
    unsigned m = 0;
#pragma unroll
    for (int b = 0; b < 8; b++) m ^= (0u - ((s >> b) & 1u)) & c[b];
    return m;
}

__device__ __forceinline__ void const_products(unsigned v, unsigned prim, unsigned (&c)[8])
{
    c[0] = v;
#pragma unroll
    for (int b = 1; b < 8; b++) c[b] = xtime(c[b - 1], prim);
}

// the xor over the wave of a byte per lane, as a scalar
__device__ __forceinline__ unsigned wave_xor8(unsigned v)
{
    unsigned d = 0;
#pragma unroll
    for (int b = 0; b < 8; b++) d |= (unsigned)(__builtin_popcountll(__ballot((v >> b) & 1u)) & 1) << b;
    return d;
}

__device__ __forceinline__ unsigned lane_up(unsigned v, unsigned lane)      // lane l gets lane l - 1's, lane 0 gets 0
{
    const unsigned t = (unsigned)__shfl_up((int)v, 1);
    return lane ? t : 0u;
}

__device__ __forceinline__ unsigned lane_read(unsigned v, int l) { return (unsigned)__builtin_amdgcn_readlane((int)v, l); }

__device__ __forceinline__ unsigned row_byte(unsigned rowreg, int j) { return (lane_read(rowreg, j >> 2) >> (8 * (j & 3))) & 0xffu; }

__device__ __forceinline__ unsigned inv254(unsigned a, unsigned prim)
{
    unsigned s = reed_mul(a, a, prim), r = s;
#pragma unroll
    for (int i = 0; i < 6; i++) {
        s = reed_mul(s, s, prim);
        r = reed_mul(r, s, prim);
    }
    return r;
}

// where byte q of a frame or a payload lies among the rows: codeword q mod depth, position q / depth
__device__ __forceinline__ unsigned row_at(unsigned q, const ReedArgs &a)
{
    const unsigned j = (q * a.recip) >> 16;
    return (q - j * (unsigned)a.depth) * REED_ROW + j;
}

// nbytes bytes at src into the rows; wh: the whitening bytes or null
__device__ __forceinline__ void load_rows(const uint8_t *__restrict__ src, unsigned nbytes, const uint8_t *__restrict__ wh, uint8_t *rows,
                                          const ReedArgs &a, unsigned tid)
{
    const unsigned head = min(nbytes, (unsigned)((0u - (unsigned)reinterpret_cast<uintptr_t>(src)) & 3u));
    const unsigned nd = (nbytes - head) >> 2, tail0 = head + 4 * nd;
    const uint32_t *__restrict__ s32 = reinterpret_cast<const uint32_t *>(src + head);
    const uint32_t *__restrict__ w32 = wh ? reinterpret_cast<const uint32_t *>(wh + (REED_TAB_WHITEN4 - REED_TAB_WHITEN) + head * REED_WHITEN_ROW) : nullptr;
    for (unsigned m = tid; m < nd; m += T) {
        unsigned v = s32[m];
        if (w32) v ^= w32[m];
#pragma unroll
        for (unsigned c = 0; c < 4; c++) rows[row_at(head + 4 * m + c, a)] = (uint8_t)(v >> (8 * c));
    }
    for (unsigned e = tid; e < head + (nbytes - tail0); e += T) {
        const unsigned q = e < head ? e : tail0 + (e - head);
        rows[row_at(q, a)] = (uint8_t)(src[q] ^ (wh ? wh[q] : 0));
    }
}

// nbytes bytes of the rows (zeros with `zero`) to dst, exactly those
__device__ __forceinline__ void store_rows(uint8_t *__restrict__ dst, unsigned nbytes, const uint8_t *__restrict__ wh, const uint8_t *rows, bool zero,
                                           const ReedArgs &a, unsigned tid)
{
    const unsigned head = min(nbytes, (unsigned)((0u - (unsigned)reinterpret_cast<uintptr_t>(dst)) & 3u));
    const unsigned nd = (nbytes - head) >> 2, tail0 = head + 4 * nd;
    uint32_t *__restrict__ d32 = reinterpret_cast<uint32_t *>(dst + head);
    const uint32_t *__restrict__ w32 = wh ? reinterpret_cast<const uint32_t *>(wh + (REED_TAB_WHITEN4 - REED_TAB_WHITEN) + head * REED_WHITEN_ROW) : nullptr;
    for (unsigned m = tid; m < nd; m += T) {
        unsigned v = 0;
        if (!zero) {
#pragma unroll
            for (unsigned c = 0; c < 4; c++) v |= (unsigned)rows[row_at(head + 4 * m + c, a)] << (8 * c);
        }
        if (w32) v ^= w32[m];
        d32[m] = v;
    }
    for (unsigned e = tid; e < head + (nbytes - tail0); e += T) {
        const unsigned q = e < head ? e : tail0 + (e - head);
        dst[q] = (uint8_t)((zero ? 0u : rows[row_at(q, a)]) ^ (wh ? wh[q] : 0));
    }
}

// One wave, one codeword in its row: the row becomes the codeword within distance t and the distance is returned, or -1 and
// the row stays.
__device__ int decode_word(uint8_t *row, const ReedArgs &a, unsigned lane)
{
    const unsigned prim = (unsigned)a.prim;
    const int n = a.n, np = a.n_par, t = a.t;
    const unsigned rowreg = reinterpret_cast<const uint32_t *>(row)[lane];
    unsigned S = 0;
    {
        unsigned c[8];
        const_products((int)lane < np ? a.tab[REED_TAB_ROOT + lane] : 0u, prim, c);
        for (int j = 0; j < n; j++) S = mul_const(c, S) ^ row_byte(rowreg, j);
    }
    if ((int)lane >= np) S = 0;
    if (__ballot(S != 0) == 0ull) return 0;

    // C: Lambda up to a factor; Bs: x^m B; lane l the coefficient of x^l.  Srev: S_(r-l) in lane l.
    unsigned C = lane == 0, Bs = lane == 1, Srev = 0, bq = 1;
    int L = 0;
    for (int r = 0; r < np; r++) {
        Srev = lane_up(Srev, lane);
        if (lane == 0) Srev = lane_read(S, r);
        const unsigned d = wave_xor8(reed_mul(C, Srev, prim));
        const unsigned Cn = reed_mul(C, bq, prim) ^ reed_mul(Bs, d, prim);
        const bool grow = d != 0 && 2 * L <= r;
        Bs = lane_up(grow ? C : Bs, lane);
        if (grow) {
            L = r + 1 - L;
            bq = d;
        }
        C = Cn;
    }
    const unsigned long long nzc = __ballot(C != 0);        // never empty: the constant term is a product of nonzero factors
    bool ok = L <= t && 63 - __builtin_clzll(nzc | 1ull) == L;

    // Omega = S Lambda mod x^t, lane i the coefficient of x^i
    unsigned Om = 0;
    {
        unsigned Ssh = S;
        for (int l = 0; l <= t; l++) {
            Om ^= reed_mul(Ssh, lane_read(C, l), prim);
            Ssh = lane_up(Ssh, lane);
        }
    }
    unsigned mag[4] = {0, 0, 0, 0};
    bool isroot[4] = {false, false, false, false};
    int nroots = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        if (64 * q < n) {
            const int p = 64 * q + (int)lane;
            const unsigned z = p < n ? a.tab[REED_TAB_ZINV + p] : 0u;
            unsigned ev = 0;
            for (int l = t; l >= 0; l--) ev = reed_mul(ev, z, prim) ^ lane_read(C, l);
            isroot[q] = p < n && ev == 0;
            const unsigned long long rb = __ballot(isroot[q]);
            nroots += __builtin_popcountll(rb);
            if (rb) {
                unsigned om = 0, dv = 0;
                for (int i = t - 1; i >= 0; i--) om = reed_mul(om, z, prim) ^ lane_read(Om, i);
                const unsigned w = reed_mul(z, z, prim);
                for (int m = (t - 1) >> 1; m >= 0; m--) dv = reed_mul(dv, w, prim) ^ lane_read(C, 2 * m + 1);
                const unsigned xf = p < n ? a.tab[REED_TAB_XF + p] : 0u;
                mag[q] = reed_mul(reed_mul(om, xf, prim), inv254(dv, prim), prim);
            }
        }
    }
    ok = ok && nroots == L;
    if (!ok) return -1;
#pragma unroll
    for (int q = 0; q < 4; q++)
        if (isroot[q]) row[64 * q + (int)lane] ^= (uint8_t)mag[q];
    return L;
}

// One wave, one codeword: the n_par bytes behind the k message bytes of its row
__device__ void encode_word(uint8_t *row, const ReedArgs &a, unsigned lane)
{
    const unsigned prim = (unsigned)a.prim;
    const int np = a.n_par, k = a.k;
    const unsigned rowreg = reinterpret_cast<const uint32_t *>(row)[lane];
    unsigned c[8];
    const_products((int)lane < np ? a.tab[REED_TAB_GEN + lane] : 0u, prim, c);
    unsigned R = 0;                                         // lane l: the remainder's coefficient of x^l
    for (int j = 0; j < k; j++) {
        const unsigned fb = lane_read(R, np - 1) ^ row_byte(rowreg, j);
        R = lane_up(R, lane) ^ mul_const(c, fb);
    }
    if ((int)lane < np) row[k + np - 1 - (int)lane] = (uint8_t)R;
}

__global__ __launch_bounds__(T) void reed_decode_kernel(ReedArgs a)
{
    __shared__ uint32_t s_rows32[REED_ROWS * REED_ROW / 4];
    __shared__ unsigned s_cnt[REED_WAVES], s_bad[REED_WAVES], s_up[REED_WAVES];
    uint8_t *rows = reinterpret_cast<uint8_t *>(s_rows32);
    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const long long f0 = (long long)blockIdx.x * a.fpb;
    const int nf = (int)min((long long)a.fpb, a.n_frames - f0), I = a.depth;
    const unsigned Fb = (unsigned)(I * a.n), P = (unsigned)(I * a.k);
    const uint8_t *wh = a.whiten ? a.tab + REED_TAB_WHITEN : nullptr;
    if (tid < REED_WAVES) {
        s_cnt[tid] = 0;
        s_bad[tid] = 0;
        s_up[tid] = (int)tid < nf && a.status_in && a.status_in[f0 + tid] != 0;
    }
    __syncthreads();
    for (int f = 0; f < nf; f++)
        if (!s_up[f]) load_rows(a.in + (size_t)(f0 + f) * (size_t)a.in_stride, Fb, wh, rows + f * I * REED_ROW, a, tid);
    __syncthreads();
    for (int cw = (int)wave; cw < nf * I; cw += REED_WAVES) {
        const int f = (int)(((unsigned)cw * a.recip) >> 16), i = cw - f * I;
        if (s_up[f]) continue;
        const int d = decode_word(rows + cw * REED_ROW, a, lane);
        if (lane == 0) {
            if (d < 0) atomicOr(&s_bad[f], 1u << i);
            else atomicAdd(&s_cnt[f], (unsigned)d);
        }
    }
    __syncthreads();
    for (int f = 0; f < nf; f++)
        store_rows(a.out + (size_t)(f0 + f) * (size_t)a.out_stride, P, nullptr, rows + f * I * REED_ROW, s_up[f] != 0, a, tid);
    if ((int)tid < nf) {
        const bool up = s_up[tid] != 0;
        const unsigned bad = up ? (1u << I) - 1u : s_bad[tid];
        if (a.rec) {
            a.rec[2 * (f0 + tid)] = up ? 0u : s_cnt[tid];
            a.rec[2 * (f0 + tid) + 1] = bad;
        }
        if (a.status) a.status[f0 + tid] = up ? REED_UPSTREAM : bad ? REED_UNCORRECTABLE : REED_OK;
    }
}

__global__ __launch_bounds__(T) void reed_encode_kernel(ReedArgs a)
{
    __shared__ uint32_t s_rows32[REED_ROWS * REED_ROW / 4];
    uint8_t *rows = reinterpret_cast<uint8_t *>(s_rows32);
    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const long long f0 = (long long)blockIdx.x * a.fpb;
    const int nf = (int)min((long long)a.fpb, a.n_frames - f0), I = a.depth;
    const unsigned Fb = (unsigned)(I * a.n), P = (unsigned)(I * a.k);
    const uint8_t *wh = a.whiten ? a.tab + REED_TAB_WHITEN : nullptr;
    for (int f = 0; f < nf; f++) load_rows(a.in + (size_t)(f0 + f) * (size_t)a.in_stride, P, nullptr, rows + f * I * REED_ROW, a, tid);
    __syncthreads();
    for (int cw = (int)wave; cw < nf * I; cw += REED_WAVES) encode_word(rows + cw * REED_ROW, a, lane);
    __syncthreads();
    for (int f = 0; f < nf; f++) store_rows(a.out + (size_t)(f0 + f) * (size_t)a.out_stride, Fb, wh, rows + f * I * REED_ROW, false, a, tid);
}

unsigned reed_grid(const ReedArgs &a) { return (unsigned)((a.n_frames + a.fpb - 1) / a.fpb); }

}  // namespace

int launch_reed_decode(const ReedArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(reed_decode_kernel, dim3(reed_grid(a)), dim3(T), 0, st, a);
    SFE_HIP(hipGetLastError());
    return SFE_OK;
}

int launch_reed_encode(const ReedArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(reed_encode_kernel, dim3(reed_grid(a)), dim3(T), 0, st, a);
    SFE_HIP(hipGetLastError());
    return SFE_OK;
}

}  // namespace sfe
