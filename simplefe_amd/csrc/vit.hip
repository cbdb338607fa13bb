// vit.hip -- soft-decision Viterbi decoder (sfe_dsp_vit_*): per burst n_soft soft values -- float32, or the components of
// the symbols the burst demodulator wrote -- become ceil(n_info / 8) payload bytes, a record (the end state's metric, the
// count of positions that disagree with the decoded word) and a status (include/sfe_dsp.h states the law;
// api_vit.hip is its host twin, whose bits these are).
//
// ONE WAVE PER BURST, up to four bursts per workgroup, no workgroup barrier anywhere: a wave's LDS is its own.
//   soft      the burst's soft values, lanes along the positions (t, j): the finite check, and -- where the burst's LDS
//             holds them -- the copy into LDS with +0 at the punctured positions, so that a step reads its n values at
//             t n + j, the same address in every lane (a broadcast).  Otherwise each lane fetches the n values of one of the
//             next 64 steps and a step takes them out of that lane's registers.
//   step      a lane is a state (K <= 7), two (K = 8) or four (K = 9): state i 64 + lane sits in register i.  The register
//             of state s' after the step is s' itself, so s' IS the shift register of the branch from p0 = s' >> 1, and
//             s' | 2^(K-1) that of the branch from p1: the sign masks of the two branches' labels are 2 n words a lane
//             keeps for the whole burst.  A lane forms its two branch sums itself, left to right -- 2 (n - 1) additions,
//             fewer than the 2^n (n - 1) of a table of every label.  The predecessors' metrics come
//             through ds_bpermute (__shfl): p0 is lane (s' >> 1) & 63 of register s' >> 7, p1 the same lane half the
//             registers on (K <= 7: lane p0 | S/2).  The decisions leave as one ballot word per 64 states, stored by lane 0.
//   end       state 0, or the first state of the largest metric: a six-step butterfly on (metric, index).
//   traceback lane 0 walks the T ballot words back, one dependent LDS read per step, and packs the bits in LDS.
//   out       the wave stores the bytes, then re-encodes lanes along t from the packed bits and counts the kept positions
//             whose soft value's sign disagrees.
// Additions and comparisons only, each one IEEE operation: the bits are the host plan's.
#include <cfloat>

#include "vit.h"

namespace sfe {

namespace {

// LDS written by one lane of a wave and read by another: the wave's LDS operations complete in order, so only the
// compiler has to be kept from moving them across this point.
__device__ inline void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ inline bool finite32(float v) { return fabsf(v) <= FLT_MAX; }

__device__ inline unsigned long long below(int n) { return n >= 64 ? ~0ull : ((1ull << n) - 1ull); }   // bits 0 .. n - 1, n >= 0

// position (t, j) with tp = t mod P and per = t / P: is it transmitted, and as which soft value of the burst
__device__ inline bool kept_at(unsigned long long lo, unsigned long long hi, int per_period, int tp, int per, int j, int *idx)
{
    const int bit = 4 * tp + j;
    const unsigned long long w = bit < 64 ? lo : hi;
    const int ahead = bit < 64 ? __popcll(lo & below(bit)) : __popcll(lo) + __popcll(hi & below(bit - 64));
    *idx = per * per_period + ahead;
    return (w >> (bit & 63)) & 1ull;
}

__device__ inline float flip(float r, unsigned mask) { return __uint_as_float(__float_as_uint(r) ^ mask); }

template <int NG, int SPL>
__global__ __launch_bounds__(64 * VIT_MAX_WAVES) void vit_kernel(VitArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = (int)threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const long long b = (long long)blockIdx.x * a.waves + wave;
    if (b >= a.n_bursts) return;
    const int K = a.K, S = 1 << (K - 1), T = a.T, n_info = a.n_info, nbytes = (n_info + 7) >> 3, P = a.P;
    char *mine = smem + (size_t)wave * vit_burst_bytes(K, NG, T, n_info);
    unsigned long long *surv = reinterpret_cast<unsigned long long *>(mine);               // [T][SPL]
    uint8_t *pk = reinterpret_cast<uint8_t *>(mine + vit_surv_bytes(K, T));                // the packed payload
    float *soft = reinterpret_cast<float *>(mine + vit_base_bytes(K, T, n_info));          // [T][NG] (staged launches only)
    const float *row = a.in + b * a.in_stride + a.in_off;
    uint8_t *out = a.bits + b * a.out_stride;

    // what a burst without an answer gets: bytes of 0, the record (quiet NaN, 0), its status
    auto fail = [&](int st) {
        for (int i = lane; i < nbytes; i += 64) out[i] = 0;
        if (a.rec && lane == 0) a.rec[2 * b] = VIT_QNAN, a.rec[2 * b + 1] = 0u;
        if (a.status && lane == 0) a.status[b] = st;
    };
    if (a.status_in && a.status_in[b] != 0) return fail(VIT_UPSTREAM);

    // ---- the soft values: finite check, and the copy into LDS with the punctured positions filled in
    int bad = 0;
    if (a.staged) {
        for (int q = lane; q < T * NG; q += 64) {
            const int t = q / NG, j = q - t * NG, per = t / P, tp = t - per * P;
            int idx;
            float v = 0.0f;
            if (kept_at(a.keep_lo, a.keep_hi, a.per_period, tp, per, j, &idx)) v = row[(long long)idx * a.in_mul];
            bad |= !finite32(v);
            soft[q] = v;
        }
    } else {
        for (int i = lane; i < a.n_soft; i += 64) bad |= !finite32(row[(long long)i * a.in_mul]);
    }
    if (__any(bad)) return fail(VIT_NOT_FINITE);
    wave_sync();

    // ---- the sign masks of a lane's incoming branches: constants of (K, gen)
    unsigned m0[SPL][NG], m1[SPL][NG];
#pragma unroll
    for (int i = 0; i < SPL; i++) {
        const unsigned reg = (unsigned)(i * 64 + lane);
#pragma unroll
        for (int j = 0; j < NG; j++) {
            m0[i][j] = (unsigned)(__popc(reg & a.gen[j]) & 1) << 31;
            m1[i][j] = (unsigned)(__popc((reg | (unsigned)S) & a.gen[j]) & 1) << 31;
        }
    }
    const float ninf = -__builtin_inff();
    float pm[SPL];
#pragma unroll
    for (int i = 0; i < SPL; i++) pm[i] = (i == 0 && lane == 0) ? 0.0f : ninf;
    const int src0 = lane >> 1;                                         // the lane of p0 (registers 2i) ...
    const int src1 = SPL == 1 ? (src0 | (S >> 1)) : (src0 | 32);        // ... and of p1 (K <= 7), or of p0 for registers 2i + 1
    const unsigned long long live = S >= 64 ? ~0ull : ((1ull << S) - 1ull);

    // ---- T add-compare-select steps
    float ahead[NG] = {};               // unstaged: the soft values of step (t & ~63) + lane
    for (int t = 0; t < T; t++) {
        float r[NG];
        if (a.staged) {
#pragma unroll
            for (int j = 0; j < NG; j++) r[j] = soft[t * NG + j];
        } else {
            if ((t & 63) == 0) {
                const int tt = t + lane, per = tt / P, tp = tt - per * P;
#pragma unroll
                for (int j = 0; j < NG; j++) {
                    int idx;
                    ahead[j] = 0.0f;
                    if (tt < T && kept_at(a.keep_lo, a.keep_hi, a.per_period, tp, per, j, &idx)) ahead[j] = row[(long long)idx * a.in_mul];
                }
            }
#pragma unroll
            for (int j = 0; j < NG; j++) r[j] = __shfl(ahead[j], t & 63);
        }
        float nw[SPL];
#pragma unroll
        for (int i = 0; i < SPL; i++) {
            float bm0 = flip(r[0], m0[i][0]), bm1 = flip(r[0], m1[i][0]);
#pragma unroll
            for (int j = 1; j < NG; j++) {
                bm0 = bm0 + flip(r[j], m0[i][j]);
                bm1 = bm1 + flip(r[j], m1[i][j]);
            }
            float a0, a1;
            if (SPL == 1) {
                a0 = __shfl(pm[0], src0);
                a1 = __shfl(pm[0], src1);
            } else {
                a0 = __shfl(pm[i >> 1], (i & 1) ? src1 : src0);
                a1 = __shfl(pm[(i >> 1) + SPL / 2], (i & 1) ? src1 : src0);
            }
            const float c0 = a0 + bm0, c1 = a1 + bm1;
            const bool d = c1 > c0;
            nw[i] = d ? c1 : c0;
            const unsigned long long word = __ballot(d) & live;
            if (lane == 0) surv[t * SPL + i] = word;
        }
#pragma unroll
        for (int i = 0; i < SPL; i++) pm[i] = (SPL > 1 || lane < S) ? nw[i] : ninf;
    }

    // ---- the end state and its metric
    float bv = pm[0];
    int end = 0;
    if (a.terminated) {
        bv = __shfl(pm[0], 0);
    } else {
        int bi = lane;
#pragma unroll
        for (int i = 1; i < SPL; i++)
            if (pm[i] > bv) bv = pm[i], bi = i * 64 + lane;
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            const float ov = __shfl_xor(bv, m);
            const int oi = __shfl_xor(bi, m);
            if (ov > bv || (ov == bv && oi < bi)) bv = ov, bi = oi;
        }
        end = bi & (S - 1);
    }

    // ---- traceback: T dependent LDS reads by one lane
    if (lane == 0) {
        int s = end;
        unsigned acc = 0;
        for (int t = T - 1; t >= 0; t--) {
            if (t < n_info) {
                acc |= (unsigned)(s & 1) << (7 - (t & 7));
                if ((t & 7) == 0) pk[t >> 3] = (uint8_t)acc, acc = 0;
            }
            const unsigned d = (unsigned)(surv[t * SPL + (s >> 6)] >> (s & 63)) & 1u;
            s = (s >> 1) | (int)(d << (K - 2));
        }
    }
    wave_sync();

    // ---- the bytes, and the positions that disagree with the decoded word
    for (int i = lane; i < nbytes; i += 64) out[i] = pk[i];
    unsigned cnt = 0;
    for (int t = lane; t < T; t += 64) {
        unsigned reg = 0;
        for (int k = 0; k < K; k++) {
            const int u = t - k;
            if (u >= 0 && u < n_info) reg |= (unsigned)((pk[u >> 3] >> (7 - (u & 7))) & 1) << k;
        }
        const int per = t / P, tp = t - per * P;
#pragma unroll
        for (int j = 0; j < NG; j++) {
            float v = 0.0f;             // a punctured position is +0: it agrees
            if (a.staged) {
                v = soft[t * NG + j];
            } else {
                int idx;
                if (kept_at(a.keep_lo, a.keep_hi, a.per_period, tp, per, j, &idx)) v = row[(long long)idx * a.in_mul];
            }
            cnt += (__popc(reg & a.gen[j]) & 1) ? (v > 0.0f) : (v < 0.0f);
        }
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) cnt += __shfl_xor(cnt, m);
    if (lane == 0) {
        if (a.rec) a.rec[2 * b] = __float_as_uint(bv), a.rec[2 * b + 1] = cnt;
        if (a.status) a.status[b] = VIT_OK;
    }
}

template <int NG, int SPL>
int launch_one(const VitArgs &a, size_t lds, hipStream_t st, bool prepare_only)
{
    if (prepare_only) {
        if (lds > 65536)
            SFE_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&vit_kernel<NG, SPL>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        return SFE_OK;
    }
    const dim3 grid((unsigned)((a.n_bursts + a.waves - 1) / a.waves));
    hipLaunchKernelGGL((vit_kernel<NG, SPL>), grid, dim3(64 * a.waves), lds, st, a);
    SFE_HIP(hipGetLastError());
    return SFE_OK;
}

template <int NG>
int launch_n(const VitArgs &a, size_t lds, hipStream_t st, bool prepare_only)
{
    switch (vit_words(a.K)) {
    case 1: return launch_one<NG, 1>(a, lds, st, prepare_only);
    case 2: return launch_one<NG, 2>(a, lds, st, prepare_only);
    default: return launch_one<NG, 4>(a, lds, st, prepare_only);
    }
}

}  // namespace

int launch_vit(const VitArgs &a, hipStream_t st, bool prepare_only)
{
    const size_t lds = (size_t)a.waves * vit_burst_bytes(a.K, a.n_gen, a.T, a.n_info);
    switch (a.n_gen) {
    case 2: return launch_n<2>(a, lds, st, prepare_only);
    case 3: return launch_n<3>(a, lds, st, prepare_only);
    default: return launch_n<4>(a, lds, st, prepare_only);
    }
}

}  // namespace sfe
