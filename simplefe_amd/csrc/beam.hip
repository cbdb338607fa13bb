// beam.hip -- multi-stream beamformer / stream-mixing bank (sfe_dsp_beam_*): B beams out of S streams, per band.
//
//   y_{b,k}[m] = sum_s  W_k[b][s] x_{s,k}[m] + V_k[b][s] conj(x_{s,k}[m])
//
// The host (api_beam.hip) turns a band's (W, V) into one real matrix R of 2B x 2S float32 -- row 2b / 2b+1 the real /
// imaginary part of beam b, column 2s / 2s+1 those of stream s -- and the law is the real product Y = R X on the matrix
// pipe: interleaved cf32 IS X's layout (K-rows 2s and 2s+1 of column m are the two floats of sample m of stream s).
//
// v_mfma_f32_16x16x4_f32: D[16 x 16] += A[16 x 4] B[4 x 16], A = 16 rows of R, B = 16 consecutive samples (the columns),
// K = four floats of X.  Lane l = 16 kq + j loads ONE cf32 sample -- stream 4p + kq, sample j of the column block -- and
// uses it in two K-steps: step 2p takes the real parts of streams 4p .. 4p+3, step 2p+1 their imaginary parts.  So a
// sample is fetched once, by one lane of one wave, as one 8-byte load (16 lanes: 128 contiguous bytes of a stream), and
// never crosses lanes; the order of the 2S terms of an output float is
//     Re x_0, Re x_1, Re x_2, Re x_3, Im x_0, .. Im x_3, Re x_4, ..       (a k-ordered fmaf chain from zero)
// whatever the sample's place in a call, a tile or a buffer.  R is laid out for that lane order by the host
// (beam.h: beam_frag_at) and sits in LDS, read one float per lane and K-step (conflict-free: consecutive lanes,
// consecutive words) and reused over the NB column blocks of a tile.
// D: lane l, register i is row 16 rt + 4 kq + i, column j: the lane holds beams 8 rt + 2 kq and 8 rt + 2 kq + 1 of its
// sample as two cf32 values and stores them as such (16 lanes: 128 contiguous bytes of a beam).
//
// WAVE-granular: every wave of a workgroup walks its own tiles of 16 NB samples of the workgroup's band and computes
// ALL 2B rows of them; nothing but R is shared, so there is no barrier after R is in place and no input byte is read
// twice.  The tail of a call runs the same instructions with the loads and stores of samples >= n_in masked; streams
// >= S and the columns of R beyond 2S are zero ON BOTH SIDES (a padding lane loads nothing and multiplies 0 by 0), K
// pairs and row tiles that are all padding are skipped.
// Classes: KP = pairs of K-steps, RT = row tiles, each a power of two (beam.h); 5 x 4 classes x {cf32, u8 pairs}.
#include <atomic>

#include "beam.h"

namespace sfe {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct BeamArgs {
    const void *in;
    v2f *out;
    const float *frag;          // [M][RT][2 KP][64]
    long long in_stride, out_stride, n_in, tiles;
    int S, B, M;
};

constexpr int beam_nb(int KP, int RT) { return (KP >= 16 || RT >= 8) ? 2 : 4; }     // column blocks of 16 samples per tile

template <int KP, int RT, bool U8>
__global__ __launch_bounds__(256) void beam_kernel(BeamArgs a)
{
    constexpr int NB = beam_nb(KP, RT), KS = 2 * KP, NF = RT * KS * 64;
    __shared__ float Rf[NF];
    const unsigned tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, kq = lane >> 4;
    const size_t band = blockIdx.y;
    const float *frag = a.frag + band * NF;
    for (unsigned i = tid; i < (unsigned)NF; i += 256) Rf[i] = frag[i];
    __syncthreads();

    const int S = a.S, B = a.B;
    const long long n = a.n_in;
    const long long wstride = (long long)gridDim.x * 4;
    for (long long t = (long long)blockIdx.x * 4 + wave; t < a.tiles; t += wstride) {
        const long long m0 = t * (16 * NB) + j;
        // the masks "stream kq' < S" and "beam < B" are the same for every tile: recomputed per tile (two compares)
        // instead of kept, 2 KP + 2 RT wave masks in scalar registers, across the loop
        int kq_in = (int)kq, kq_out = (int)kq;
        asm volatile("" : "+v"(kq_in), "+v"(kq_out));
        // this lane's samples: stream 4p + kq, column blocks 0 .. NB-1; zero where there is no stream or no sample
        v2f x[KP][NB];
#pragma unroll
        for (int p = 0; p < KP; p++) {
            const int s = 4 * p + kq_in;
            const size_t row = ((size_t)s * a.M + band) * (size_t)a.in_stride;
#pragma unroll
            for (int nb = 0; nb < NB; nb++) {
                const long long m = m0 + 16 * nb;
                x[p][nb] = v2f{0.0f, 0.0f};
                if (s < S && m < n) {
                    if constexpr (U8) {
                        const unsigned w = __builtin_nontemporal_load(static_cast<const unsigned short *>(a.in) + row + m);
                        x[p][nb] = v2f{u8_to_f32(w & 0xffu), u8_to_f32(w >> 8)};
                    } else {
                        x[p][nb] = __builtin_nontemporal_load(static_cast<const v2f *>(a.in) + row + m);
                    }
                }
            }
        }

        f32x4 acc[RT][NB];
#pragma unroll
        for (int rt = 0; rt < RT; rt++)
#pragma unroll
            for (int nb = 0; nb < NB; nb++) acc[rt][nb] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int p = 0; p < KP; p++) {
            if (4 * p >= S) continue;               // the same for every lane
#pragma unroll
            for (int part = 0; part < 2; part++) {
#pragma unroll
                for (int rt = 0; rt < RT; rt++) {
                    if (8 * rt >= B) continue;
                    const float r = Rf[(rt * KS + 2 * p + part) * 64 + lane];
#pragma unroll
                    for (int nb = 0; nb < NB; nb++)
                        acc[rt][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(r, part ? x[p][nb].y : x[p][nb].x, acc[rt][nb], 0, 0, 0);
                }
            }
        }

#pragma unroll
        for (int rt = 0; rt < RT; rt++) {
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const int b = 8 * rt + 2 * kq_out + h;
                if (b >= B) continue;
                v2f *orow = a.out + ((size_t)b * a.M + band) * (size_t)a.out_stride;
#pragma unroll
                for (int nb = 0; nb < NB; nb++) {
                    const long long m = m0 + 16 * nb;
                    if (m < n) __builtin_nontemporal_store(v2f{acc[rt][nb][2 * h], acc[rt][nb][2 * h + 1]}, orow + m);
                }
            }
        }
    }
}

template <int KP, int RT, bool U8>
int beam_launch(BeamArgs a, hipStream_t st)
{
    constexpr int NB = beam_nb(KP, RT);
    a.tiles = (a.n_in + 16 * NB - 1) / (16 * NB);
    // workgroups: what the device holds at once, shared over the bands (every workgroup loads its band's matrix once)
    static std::atomic<int> per_cu_cache{0};
    int per_cu = per_cu_cache.load(std::memory_order_relaxed);
    if (per_cu == 0) {
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, beam_kernel<KP, RT, U8>, 256, 0) != hipSuccess || per_cu < 1) per_cu = 1;
        per_cu_cache.store(per_cu, std::memory_order_relaxed);
    }
    long long gx = (a.tiles + 3) / 4;
    const long long cap = ((long long)device_cu_count() * per_cu + a.M - 1) / a.M;
    if (gx > cap) gx = cap;
    hipLaunchKernelGGL((beam_kernel<KP, RT, U8>), dim3((unsigned)gx, (unsigned)a.M), dim3(256), 0, st, a);
    SFE_HIP(hipGetLastError());
    return SFE_OK;
}

template <int KP, bool U8>
int beam_launch_rt(int RT, const BeamArgs &a, hipStream_t st)
{
    switch (RT) {
    case 1: return beam_launch<KP, 1, U8>(a, st);
    case 2: return beam_launch<KP, 2, U8>(a, st);
    case 4: return beam_launch<KP, 4, U8>(a, st);
    case 8: return beam_launch<KP, 8, U8>(a, st);
    }
    set_error("beam: no kernel for %d row tiles", RT);
    return SFE_EINVAL;
}

template <bool U8>
int beam_launch_kp(int KP, int RT, const BeamArgs &a, hipStream_t st)
{
    switch (KP) {
    case 1: return beam_launch_rt<1, U8>(RT, a, st);
    case 2: return beam_launch_rt<2, U8>(RT, a, st);
    case 4: return beam_launch_rt<4, U8>(RT, a, st);
    case 8: return beam_launch_rt<8, U8>(RT, a, st);
    case 16: return beam_launch_rt<16, U8>(RT, a, st);
    }
    set_error("beam: no kernel for %d K-step pairs", KP);
    return SFE_EINVAL;
}

}  // namespace

int launch_beam(int u8, const void *in, long long in_stride, v2f *out, long long out_stride, const float *frag, long long n_in,
                int S, int B, int M, hipStream_t st)
{
    const BeamArgs a{in, out, frag, in_stride, out_stride, n_in, 0, S, B, M};
    const int KP = beam_kp(S), RT = beam_rt(B);
    return u8 ? beam_launch_kp<true>(KP, RT, a, st) : beam_launch_kp<false>(KP, RT, a, st);
}

}  // namespace sfe
