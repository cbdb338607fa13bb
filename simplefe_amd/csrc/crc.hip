// crc.hip -- the kernels of the frame check (sfe_dsp_crc_*, include/sfe_dsp.h): payloads to scrambled frames with their CRC
// behind them (append), channel frames to payloads with a record and a status (check), by the law of crc_law.h.  Integer work
// only; the host plan (api_crc.hip) states the same law a byte at a time, and the two give the same bytes because the law
// determines them.
//
// A CRC is a serial recurrence over a frame's bytes, so one frame is spread over the T lanes of its group -- a wave (rows up
// to CRC_SHORT_MAX bytes, CRC_SHORT_FPB frames per workgroup) or a workgroup of CRC_LONG_T threads (longer rows):
//   - the frame's whole dwords, in frame coordinates, are dealt round robin: in round i lane l takes dword i T + l - pad, a
//     contiguous 4-byte piece, and the wave's pieces of a round are 256 contiguous bytes.  pad = rounds T - nd zero dwords
//     stand in front of the frame, which a register started at zero does not see, so every lane runs the same rounds and
//     a lane's place in the last round does not depend on the payload's length;
//   - a row starts at any byte address: the pieces are read and stored as dwords at whatever address they have, and the
//     sequence, which the handle keeps in frame coordinates, is met in aligned dwords;
//   - each lane forms its pieces' remainder from a zero register: A = A x^(32 T) + D mod G' per round, D the piece with its
//     first byte on top (a byte swap; where the model reflects, one bit reversal of the dword does both).  The product with
//     the constant x^(32 T) is table-free: its 32 columns x^(b + 32 T) are uniform, one (bit-extract, and, xor) per bit;
//   - the lanes are folded once per frame: lane l's register times its weight x^(32 (T - l)) (shift and xor, crc_mulmod),
//     xor over the wave by lane exchanges, over the waves of a long frame's workgroup through 16 words of LDS;
//   - the up to 3 bytes behind the last dword go through the register bit by bit, a non-zero init is one more term
//     (init_term), and the register is finished as the law says;
//   - the de-scrambling xor and the payload's copy ride in the same pass: every dword is read once and stored once.
// No scratch, no atomics, no tables of bytes: nothing is looked up by data.
#include "crc.h"

namespace sfe {
namespace {

constexpr int CRC_GRID_X_LOG2 = 20;

__device__ __forceinline__ uint32_t load32(const uint8_t *p)
{
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}
__device__ __forceinline__ void store32(uint8_t *p, uint32_t v) { __builtin_memcpy(p, &v, 4); }

// A times the constant whose products with x^b are col[b]
__device__ __forceinline__ uint32_t times_const(const uint32_t (&col)[32], uint32_t A)
{
    uint32_t r = 0;
#pragma unroll
    for (int b = 0; b < 32; b++) r ^= (uint32_t)((int32_t)(A << (31 - b)) >> 31) & col[b];
    return r;
}

__device__ __forceinline__ uint32_t wave_xor(uint32_t v)
{
#pragma unroll
    for (int s = 32; s; s >>= 1) v ^= (uint32_t)__shfl_xor((int)v, s);
    return v;
}

// frame f by the group of T lanes that thread tid belongs to; col: the class's columns, weight: the lane's; s_part: one word
// per wave of a long frame's workgroup
template <int T, bool CHECK>
__device__ __forceinline__ void one_frame(const CrcArgs &a, long long f, unsigned tid, const uint32_t (&col)[32], uint32_t weight, uint32_t *s_part)
{
    constexpr int WAVES = T / 64;
    const unsigned t = tid % T;
    const CrcLaw &c = a.law;
    const unsigned P = (unsigned)c.payload, nt = (unsigned)c.tail_bytes(), nd = P >> 2;
    const uint8_t *__restrict__ src = a.in + (size_t)f * (size_t)a.in_stride;
    uint8_t *__restrict__ dst = a.out ? a.out + (size_t)f * (size_t)a.out_stride : nullptr;
    const uint8_t *__restrict__ pn = a.pn;
    const uint32_t *__restrict__ pn32 = reinterpret_cast<const uint32_t *>(a.pn);
    if (CHECK && a.status_in && a.status_in[f] != 0) {
        if (dst) {
            for (unsigned d = t; d < nd; d += T) store32(dst + 4 * (size_t)d, 0u);
            for (unsigned q = 4 * nd + t; q < P; q += T) dst[q] = 0;
        }
        if (t == 0) {
            if (a.rec) a.rec[2 * f] = a.rec[2 * f + 1] = 0u;
            if (a.status) a.status[f] = CRC_UPSTREAM;
        }
        return;
    }
    const uint32_t polyL = c.polyL();
    const unsigned rounds = (nd + T - 1) / T, pad = rounds * T - nd;
    uint32_t A = 0;
    for (unsigned i = 0; i < rounds; i++) {
        const unsigned v = i * T + t;
        uint32_t D = 0;
        if (v >= pad) {
            const size_t d = v - pad;
            const uint32_t raw = load32(src + 4 * d), k = pn32 ? pn32[d] : 0u;
            if (dst) store32(dst + 4 * d, raw ^ k);
            const uint32_t plain = CHECK ? raw ^ k : raw;
            D = c.reflect ? crc_rev32(plain) : __builtin_bswap32(plain);
        }
        if (c.width) A = times_const(col, A) ^ D;
    }
    uint32_t R = 0;
    if (c.width) {
        R = wave_xor(crc_mulmod(A, weight, polyL));
        if (WAVES > 1) {
            if ((tid & 63u) == 0) s_part[tid >> 6] = R;
            __syncthreads();
            R = 0;
#pragma unroll
            for (int w = 0; w < WAVES; w++) R ^= s_part[w];
        }
    }
    for (unsigned q = 4 * nd; q < P; q++) {     // the bytes behind the last whole dword: every lane, the same register
        const uint32_t raw = src[q], k = pn ? pn[q] : 0u;
        if (dst && t == q - 4 * nd) dst[q] = (uint8_t)(raw ^ k);
        const uint32_t plain = CHECK ? raw ^ k : raw;
        R = crc_feed(R, c.reflect ? crc_rev8(plain) : plain, polyL);
    }
    const uint32_t crc = crc_finish(R ^ a.init_term, c);
    if (!CHECK) {
        if (t < nt) dst[P + t] = (uint8_t)(crc_tail_byte(crc, (int)t, c) ^ (pn ? pn[P + t] : 0u));
        return;
    }
    uint32_t got = 0;
    for (unsigned k = 0; k < nt; k++) got |= crc_tail_place((uint32_t)src[P + k] ^ (pn ? pn[P + k] : 0u), (int)k, c);
    if (t == 0) {
        if (a.rec) {
            a.rec[2 * f] = crc;
            a.rec[2 * f + 1] = got;
        }
        if (a.status) a.status[f] = crc == got ? CRC_OK : CRC_MISMATCH;
    }
}

// group g of the grid is (blockIdx.y << CRC_GRID_X_LOG2) + blockIdx.x: a launch of 2^31 frames stays inside the grid's limits
template <int T, int FPB, bool CHECK>
__global__ __launch_bounds__(T * FPB) void crc_kernel(CrcArgs a)
{
    __shared__ uint32_t s_part[T / 64];
    const unsigned tid = threadIdx.x;
    const uint32_t *__restrict__ tab = a.tab + (T == CRC_SHORT_T ? CRC_TAB_SHORT : CRC_TAB_LONG);
    uint32_t col[32];
#pragma unroll
    for (int b = 0; b < 32; b++) col[b] = tab[b];
    const uint32_t weight = tab[32 + tid % T];
    const long long f = (((long long)blockIdx.y << CRC_GRID_X_LOG2) + blockIdx.x) * FPB + tid / T;
    if (f < a.n_frames) one_frame<T, CHECK>(a, f, tid, col, weight, s_part);        // a whole group leaves together
}

dim3 crc_grid(long long groups)
{
    const long long X = 1ll << CRC_GRID_X_LOG2;
    return groups <= X ? dim3((unsigned)groups) : dim3((unsigned)X, (unsigned)((groups + X - 1) / X));
}

}  // namespace

int launch_crc(const CrcArgs &a, hipStream_t st)
{
    if (a.law.payload > CRC_SHORT_MAX) {
        const dim3 grid = crc_grid(a.n_frames), block(CRC_LONG_T);
        if (a.check) hipLaunchKernelGGL((crc_kernel<CRC_LONG_T, 1, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((crc_kernel<CRC_LONG_T, 1, false>), grid, block, 0, st, a);
    } else {
        const dim3 grid = crc_grid((a.n_frames + CRC_SHORT_FPB - 1) / CRC_SHORT_FPB), block(CRC_SHORT_T * CRC_SHORT_FPB);
        if (a.check) hipLaunchKernelGGL((crc_kernel<CRC_SHORT_T, CRC_SHORT_FPB, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((crc_kernel<CRC_SHORT_T, CRC_SHORT_FPB, false>), grid, block, 0, st, a);
    }
    SFE_HIP(hipGetLastError());
    return SFE_OK;
}

}  // namespace sfe
