// ldpc.hip -- the quasi-cyclic LDPC code's two kernels (sfe_dsp_ldpc_*): the layered min-sum decoder, n soft values per
// codeword -- float32, or the components of the symbols the burst demodulator wrote -- into ceil(k / 8) payload bytes, a
// record (iterations, unsatisfied checks, decisions that left the input's sign) and a status; and the encoder, ceil(k / 8)
// payload bytes into ceil(n / 8) codeword bytes.  include/sfe_dsp.h states the law, ldpc_law.h is its arithmetic -- the row
// update both sides compile -- and api_ldpc.hip holds the host plan whose bytes these are.
//
// DECODER.  A workgroup of 256 threads holds 1, 2 or 4 codewords in LDS (ldpc.h: the layout), 256, 128 or 64 threads each.
//   in       a word's threads read its n soft values once, lanes along v: the finite check and the quantiser; APP and L.
//   syndrome before the first iteration and after every one: a thread takes rows i, i + T, ... of every layer, XORs the signs
//            of the row's variables, and the word's count of unsatisfied rows is summed with an LDS atomic into the slot of
//            THAT iteration, cnt[it], so no slot is ever cleared.  It is a pass of its own: the parities a layered pass meets
//            on its way are those of sums that later layers still change, not of the decisions the law examines.
//   layer    a thread takes rows i, i + T, ... of the layer (Z > 256 strides): ldpc_row_update, two passes over the row's
//            cells in LDS.  Consecutive i are consecutive int16 of APP (from the wrap on, consecutive again) and consecutive
//            int8 of the messages.  The Z rows of a layer touch disjoint variables; ONE barrier per layer.
//   leaving  EVERY thread of the workgroup executes the same barriers: one behind each syndrome pass and one behind each
//            layer, whether its word is alive, finished or missing -- those only skip the work between them.  Behind the
//            syndrome's barrier every thread reads the cnt[it] of all the workgroup's words, so the verdict "all of them are
//            done, or it == max_iter" is the same in all 256 threads: the loop is left together.  A finished word's LDS is
//            not touched again, and its iteration count was fixed when it finished.
//   out      bytes from the signs of APP, a thread per byte; the third record word through one more LDS sum.
// ENCODER.  A workgroup per codeword.  s = A u, the syndrome of the information part, is written per block as the doubled,
// reversed bit row  srr_c[x] = s_c[-x mod Z], x in [0, 2 Z), so that for parity bit (r, i) the cyclic correlation with block
// (r, c) of the parity part's inverse is 32 positions per AND: the window of srr_c that starts at bit Z - i against the
// inverse block's words, then a population count's parity.  Bits are gathered into the codeword's words in LDS.
// No global atomics, no scratch; integer work apart from the quantiser's one multiply.
#include <cfloat>

#include "ldpc.h"

namespace sfe {

namespace {

__device__ inline unsigned wave_sum(unsigned v)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
    return v;
}

__global__ __launch_bounds__(LDPC_THREADS) void ldpc_decode_kernel(LdpcArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const LdpcLayout &l = a.lay;
    const int tid = (int)threadIdx.x, G = l.group, T = l.tpw, g = tid / T, lt = tid - g * T;
    const int n = a.n, Z = a.Z, mb = a.mb, edges = a.n_cells * Z;
    LdpcCell *cells = reinterpret_cast<LdpcCell *>(smem);
    int *row_start = reinterpret_cast<int *>(smem + l.off_rows);
    char *mine = smem + l.off_words + (size_t)g * l.word_bytes;
    int16_t *app = reinterpret_cast<int16_t *>(mine);
    int8_t *L = reinterpret_cast<int8_t *>(mine + l.off_L);
    int8_t *msg = reinterpret_cast<int8_t *>(mine + l.off_msg);
    unsigned *cnt = reinterpret_cast<unsigned *>(mine + l.off_cnt);
    const long long b0 = (long long)blockIdx.x * G, b = b0 + g;
    const bool live = b < a.n_words;

    // ---- the table, and a word's zeroed messages and counters
    for (int q = tid; q < a.n_cells; q += LDPC_THREADS) {
        const uint32_t w = a.tab[a.tab_cells + q];
        cells[q] = LdpcCell{(uint16_t)(w & 0xffffu), (uint16_t)(w >> 16)};
    }
    for (int q = tid; q <= mb; q += LDPC_THREADS) row_start[q] = (int)a.tab[q];
    {
        uint32_t *mw = reinterpret_cast<uint32_t *>(msg);
        for (int q = lt; q < (edges + 3) >> 2; q += T) mw[q] = 0u;
        for (int q = lt; q < LDPC_CNT_WORDS; q += T) cnt[q] = 0u;
    }
    __syncthreads();

    // ---- the soft values: finite check and quantiser
    const bool upstream = live && a.status_in && a.status_in[b] != 0;
    if (live && !upstream) {
        const float *row = a.in + b * a.in_stride + a.in_off;
        bool bad = false;
        for (int v = lt; v < n; v += T) {
            const float r = row[(long long)v * a.in_mul];
            const bool fin = fabsf(r) <= FLT_MAX;
            const int q = fin ? ldpc_quant(r, a.scale) : 0;
            bad |= !fin;
            app[v] = (int16_t)q;
            L[v] = (int8_t)q;
        }
        if (bad) cnt[LDPC_CNT_BAD] = 1u;
    }
    __syncthreads();

    // ---- which of the workgroup's words take no part: the same mask in every thread
    unsigned donemask = 0;
    for (int h = 0; h < G; h++) {
        const unsigned *ch = reinterpret_cast<const unsigned *>(smem + l.off_words + (size_t)h * l.word_bytes + l.off_cnt);
        const bool dead = b0 + h >= a.n_words || (a.status_in && a.status_in[b0 + h] != 0) || ch[LDPC_CNT_BAD] != 0u;
        donemask |= dead ? 1u << h : 0u;
    }
    const unsigned all = (1u << G) - 1u;
    const bool failed = (donemask >> g) & 1u;
    bool mydone = failed;
    unsigned iters = 0, unsat = 0;

    for (int it = 0;; it++) {
        if (!mydone) {
            unsigned u = 0;
            for (int r = 0; r < mb; r++) {
                const int first = row_start[r], d = row_start[r + 1] - first;
                for (int i = lt; i < Z; i += T) u += ldpc_row_parity(app, cells, first, d, Z, i);
            }
            if (u) atomicAdd(&cnt[it], u);
        }
        __syncthreads();
        for (int h = 0; h < G; h++) {
            const unsigned *ch = reinterpret_cast<const unsigned *>(smem + l.off_words + (size_t)h * l.word_bytes + l.off_cnt);
            donemask |= ch[it] == 0u ? 1u << h : 0u;
        }
        if (!mydone) {
            unsat = cnt[it], iters = (unsigned)it;
            mydone = unsat == 0u;
        }
        if (donemask == all || it == a.max_iter) break;         // the same in all 256 threads
        for (int r = 0; r < mb; r++) {
            if (!mydone) {
                const int first = row_start[r], d = row_start[r + 1] - first;
                for (int i = lt; i < Z; i += T) ldpc_row_update(app, msg, cells, first, d, Z, i, a.a, a.beta);
            }
            __syncthreads();
        }
    }

    // ---- out
    const int kb = (a.k + 7) >> 3;
    unsigned flips = 0;
    if (live) {
        uint8_t *out = a.out + b * a.out_stride;
        if (failed) {
            for (int q = lt; q < kb; q += T) out[q] = 0;
        } else {
            for (int q = lt; q < kb; q += T) {
                unsigned byte = 0;
                for (int j = 0; j < 8; j++) {
                    const int v = 8 * q + j;
                    if (v < a.k) byte |= (unsigned)(app[v] < 0) << (7 - j);
                }
                out[q] = (uint8_t)byte;
            }
            for (int v = lt; v < n; v += T) flips += L[v] != 0 && (app[v] < 0) != (L[v] < 0);
        }
    }
    flips = wave_sum(flips);
    if ((tid & 63) == 0 && flips) atomicAdd(&cnt[LDPC_CNT_FLIPS], flips);
    __syncthreads();
    if (live && lt == 0) {
        if (a.rec) {
            a.rec[3 * b] = failed ? 0u : iters;
            a.rec[3 * b + 1] = failed ? 0u : unsat;
            a.rec[3 * b + 2] = failed ? 0u : cnt[LDPC_CNT_FLIPS];
        }
        if (a.status) a.status[b] = failed ? (upstream ? LDPC_UPSTREAM : LDPC_NOT_FINITE) : (unsat == 0u ? LDPC_OK : LDPC_NOT_CONVERGED);
    }
}

__device__ inline unsigned bit_of(const uint8_t *bytes, int g) { return (bytes[g >> 3] >> (7 - (g & 7))) & 1u; }

// bit g of the MSB-first packed codeword, in the little-endian words of LDS
__device__ inline void set_bit(unsigned *words, int g)
{
    const int by = g >> 3;
    atomicOr(&words[by >> 2], 1u << (8 * (by & 3) + 7 - (g & 7)));
}

__global__ __launch_bounds__(LDPC_THREADS) void ldpc_encode_kernel(LdpcArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = (int)threadIdx.x, Z = a.Z, mb = a.mb, k = a.k, kbytes = (k + 7) >> 3, nbytes = (a.n + 7) >> 3;
    const int kblocks = a.n / Z - mb, SW = ldpc_enc_row_words(Z), Zw = a.Zw;
    uint8_t *ub = reinterpret_cast<uint8_t *>(smem);
    unsigned *srr = reinterpret_cast<unsigned *>(smem + ldpc_up4(kbytes));
    unsigned *cw = srr + mb * SW;
    const long long b = blockIdx.x;
    const uint8_t *in = a.payload + b * a.in_stride;

    for (int q = tid; q < kbytes; q += LDPC_THREADS) ub[q] = in[q];
    for (int q = tid; q < mb * SW; q += LDPC_THREADS) srr[q] = 0u;
    for (int q = tid; q < (nbytes + 3) >> 2; q += LDPC_THREADS) cw[q] = 0u;
    __syncthreads();

    // ---- the payload's k bits lead the codeword; the pad bits of its last byte are ignored
    {
        uint8_t *cwb = reinterpret_cast<uint8_t *>(cw);
        for (int q = tid; q < (k >> 3); q += LDPC_THREADS) cwb[q] = ub[q];
        if (tid == 0 && (k & 7)) cwb[k >> 3] = (uint8_t)(ub[k >> 3] & (0xff00u >> (k & 7)));
    }
    // ---- s = A u, per block row c as srr_c[x] = s_c[-x mod Z], x in [0, 2 Z)
    for (int c = 0; c < mb; c++) {
        const int first = (int)a.tab[c], last = (int)a.tab[c + 1];
        for (int x = tid; x < 2 * Z; x += LDPC_THREADS) {
            const int t = (x == 0 || x == Z) ? 0 : (x < Z ? Z - x : 2 * Z - x);
            unsigned s = 0;
            for (int q = first; q < last; q++) {
                const uint32_t w = a.tab[a.tab_cells + q];
                const LdpcCell ce{(uint16_t)(w & 0xffffu), (uint16_t)(w >> 16)};
                if ((int)ce.col < kblocks) s ^= bit_of(ub, ldpc_var(ce, Z, t));
            }
            if (s) atomicOr(&srr[c * SW + (x >> 5)], 1u << (x & 31));
        }
    }
    __syncthreads();

    // ---- p = B^-1 s: parity bit (r, i) is the parity of  sum_c  inv_{r,c} . window(srr_c, Z - i)
    for (int r = 0; r < mb; r++)
        for (int i = tid; i < Z; i += LDPC_THREADS) {
            unsigned acc = 0;
            for (int c = 0; c < mb; c++) {
                const uint32_t *q = a.tab + a.tab_inv + ((size_t)r * mb + c) * Zw;
                const unsigned *row = srr + c * SW;
                for (int w = 0; w < Zw; w++) {
                    const uint32_t qw = q[w];
                    if (qw == 0u) continue;
                    const int o = Z - i + 32 * w;
                    const unsigned long long two = ((unsigned long long)row[(o >> 5) + 1] << 32) | row[o >> 5];
                    acc ^= qw & (unsigned)(two >> (o & 31));
                }
            }
            if (__popc(acc) & 1) set_bit(cw, k + r * Z + i);
        }
    __syncthreads();

    uint8_t *out = a.out + b * a.out_stride;
    const uint8_t *cwb = reinterpret_cast<const uint8_t *>(cw);
    for (int q = tid; q < nbytes; q += LDPC_THREADS) out[q] = cwb[q];
}

}  // namespace

int launch_ldpc_decode(const LdpcArgs &a, hipStream_t st, bool prepare_only)
{
    if (prepare_only) {
        if (a.lay.lds > 65536)
            SFE_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&ldpc_decode_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)a.lay.lds));
        return SFE_OK;
    }
    const dim3 grid((unsigned)((a.n_words + a.lay.group - 1) / a.lay.group));
    hipLaunchKernelGGL(ldpc_decode_kernel, grid, dim3(LDPC_THREADS), a.lay.lds, st, a);
    SFE_HIP(hipGetLastError());
    return SFE_OK;
}

int launch_ldpc_encode(const LdpcArgs &a, hipStream_t st)
{
    const size_t lds = ldpc_enc_lds((a.k + 7) / 8, (a.n + 7) / 8, a.mb, a.Z);
    hipLaunchKernelGGL(ldpc_encode_kernel, dim3((unsigned)a.n_words), dim3(LDPC_THREADS), lds, st, a);
    SFE_HIP(hipGetLastError());
    return SFE_OK;
}

}  // namespace sfe
