// fir_plan.h -- the host arithmetic behind a FIR handle, before anything is uploaded or launched: how a tap count is cut into
// partitions for the 4096-point kernel, the overlap of a single transform that covers a filter, the spectrum tables of the
// tap partitions in the kernel's thread order, the two twiddle bases, and the size class of the variant cache's key.
// HOST ONLY (no HIP, nothing of the library's): tests/host/test_fir_plan.cpp holds every piece to a direct DFT and to the
// planner's own laws without a GPU.  api_fir.hip computes and uploads (FirTables); api_rs.hip builds the general-rate
// kernel's tables from the same two functions.  The pair type is a template parameter because the kernels' v2f lives in
// common.h, which a host program cannot include.
#pragma once
#include <math.h>
#include <stddef.h>

#include <utility>
#include <vector>

namespace sfe {

constexpr int FIR_PLAN_N = 4096;          // the transform length (common.h: FFT_N; host.h asserts they agree)
constexpr int FIR_MAX_PARTS = 1024;       // ~3.9 million taps; 32 KiB of spectrum per partition

// the overlap of one transform that covers this filter: n_taps - 1 samples of history (at least one), in rows of 256
static inline int fir_single_overlap(int n_taps)
{
    const int need = n_taps > 1 ? n_taps - 1 : 1;
    return ((need + 255) / 256) * 256;
}

// How a tap count is cut for the 4096-point kernel.  One launch with overlap hl costs ~1/(4096-hl) per
// output sample; P launches over partitions of `ovl` taps cost P/(4096-ovl) plus the read-modify-
// write of the output for every launch after the first (8 more bytes per sample: ~1/4 of a launch's
// traffic).  E.g. 3841 taps: one launch advances 256 samples per transform (16x the 256-tap work);
// two partitions of 2048 advance 2048 (2.25x).  Returns false beyond FIR_MAX_PARTS partitions.
static inline bool fir_choose_partition(int n_taps, int *ovl, int *parts)
{
    const int N = FIR_PLAN_N;
    double best = 1e300;
    *parts = 0;
    const int hl1 = fir_single_overlap(n_taps);
    if (hl1 < N) {
        best = 1.0 / (N - hl1);
        *ovl = hl1;
        *parts = 1;
    }
    for (int o = 256; o < N; o += 256) {
        const int P = (n_taps + o - 1) / o;
        if (P < 2 || P > FIR_MAX_PARTS) continue;
        const double cost = (P + 0.25 * (P - 1)) / (N - o);
        if (cost < best) {
            best = cost;
            *ovl = o;
            *parts = P;
        }
    }
    return *parts > 0;
}

// the history a handle carries per channel: what the slowest partition reaches back to, or (beyond FIR_MAX_PARTS
// partitions: direct kernel only) the single-transform overlap
static inline int fir_history_len(int n_taps)
{
    int ovl = 0, parts = 0;
    return fir_choose_partition(n_taps, &ovl, &parts) ? parts * ovl : fir_single_overlap(n_taps);
}

// what the tables are made from: n_sets tap vectors of n_taps taps (complex: interleaved pairs), one behind the other
struct FirShape {
    int n_taps, taps_complex, n_sets;
    int parts, ovl;             // partition p holds taps [p*ovl, (p+1)*ovl) (a single partition: all n_taps <= ovl+1 of them)
};

// Spectrum of each zero-padded tap partition in double precision, scaled by 1/N (blkconv.cxx:50 folds the same
// 1/fft_len into its multiply), permuted to the kernel's F3 thread order: thread t (k1 = t&15, k2 = t>>4), register
// k0 -> bin k2 + 16 k1 + 256 k0.  [set][partition][k0][t]
template <class V2>
std::vector<V2> fir_spectra(const FirShape &sh, const float *taps)
{
    const int N = FIR_PLAN_N;
    std::vector<double> c(N / 2), sn(N / 2);
    for (int m = 0; m < N / 2; m++) {
        c[m] = cos(-2.0 * M_PI * m / N);
        sn[m] = sin(-2.0 * M_PI * m / N);
    }
    // in-place radix-2 decimation-in-time FFT in double precision (forward sign): table construction
    // only, so that a filter of many partitions does not cost N * n_taps trigonometric multiplies
    auto fft = [&](std::vector<double> &re, std::vector<double> &im) {
        for (int i = 1, j = 0; i < N; i++) {
            int bit = N >> 1;
            for (; j & bit; bit >>= 1) j ^= bit;
            j ^= bit;
            if (i < j) {
                std::swap(re[i], re[j]);
                std::swap(im[i], im[j]);
            }
        }
        for (int len = 2; len <= N; len <<= 1) {
            const int half = len >> 1, step = N / len;
            for (int base = 0; base < N; base += len)
                for (int k = 0; k < half; k++) {
                    const double wr = c[k * step], wi = sn[k * step];
                    const int a = base + k, b = a + half;
                    const double xr = re[b] * wr - im[b] * wi, xi = re[b] * wi + im[b] * wr;
                    re[b] = re[a] - xr;
                    im[b] = im[a] - xi;
                    re[a] += xr;
                    im[a] += xi;
                }
        }
    };
    std::vector<V2> hs((size_t)sh.n_sets * sh.parts * 16 * 256);
    std::vector<double> hr(N), hi(N);
    for (int set = 0; set < sh.n_sets; set++) {
        const float *tp = taps + (size_t)set * sh.n_taps * (sh.taps_complex ? 2 : 1);
        for (int p = 0; p < sh.parts; p++) {
            const int first = sh.parts == 1 ? 0 : p * sh.ovl;
            const int count = sh.parts == 1 ? sh.n_taps : (sh.n_taps - first < sh.ovl ? sh.n_taps - first : sh.ovl);
            for (int n = 0; n < N; n++) {
                hr[n] = n < count ? (sh.taps_complex ? tp[2 * (first + n)] : tp[first + n]) / (double)N : 0.0;
                hi[n] = n < count && sh.taps_complex ? tp[2 * (first + n) + 1] / (double)N : 0.0;
            }
            fft(hr, hi);
            for (int t = 0; t < 256; t++)
                for (int k0 = 0; k0 < 16; k0++) {
                    const int bin = (t >> 4) + 16 * (t & 15) + 256 * k0;
                    hs[(((size_t)set * sh.parts + p) * 16 + k0) * 256 + t] = V2{(float)hr[bin], (float)hi[bin]};
                }
        }
    }
    return hs;
}

// twiddle bases, tw1 [7][256] over 4096 and tw2 [7][16] over 256: row k (1..3) = W^(e k), row k+3 = W^(4 e k); the kernel
// forms W^(e (4a+b)) as row[a+3] * row[b].  Row 0 is not read and stays zero.
template <class V2>
void fir_twiddles(std::vector<V2> &tw1, std::vector<V2> &tw2)
{
    tw1.assign(7 * 256, V2{0.0f, 0.0f});
    tw2.assign(7 * 16, V2{0.0f, 0.0f});
    for (int k = 1; k < 4; k++)
        for (int t = 0; t < 256; t++) {
            const double a = -2.0 * M_PI * (double)(t * k) / 4096.0;
            tw1[k * 256 + t] = V2{(float)cos(a), (float)sin(a)};
            tw1[(k + 3) * 256 + t] = V2{(float)cos(4.0 * a), (float)sin(4.0 * a)};
        }
    for (int k = 1; k < 4; k++)
        for (int n0 = 0; n0 < 16; n0++) {
            const double a = -2.0 * M_PI * (double)(n0 * k) / 256.0;
            tw2[k * 16 + n0] = V2{(float)cos(a), (float)sin(a)};
            tw2[(k + 3) * 16 + n0] = V2{(float)cos(4.0 * a), (float)sin(4.0 * a)};
        }
}

// the size class of the variant cache's key: floor(log2) of the transforms a call runs over all its channels
static inline int fir_size_class(long long nblk, int n_channels)
{
    int sc = 0;
    for (unsigned long long v = (unsigned long long)nblk * n_channels; v > 1; v >>= 1) sc++;
    return sc;
}

}  // namespace sfe
