// occ_law.h -- the law of the spectrum occupancy detector (sfe_dsp_occ_*, include/sfe_dsp.h), compiled by occ.hip for the
// device, by api_occ.hip for sfe_dsp_occ_plan on the host, and by tests/host/test_occ_law.cpp with a plain host compiler.
// The pieces the two sides share are the functions of the first half: the order of the keys, the threshold, the fold steps
// and the peak's order.  The second half is the host's serial statement of the whole law on one row, occ_plan_row.
// There is nothing here for a compiler to contract: the one multiply that feeds an add is the explicit fmaf of the moment.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define OCC_HD __host__ __device__
#else
#define OCC_HD
#endif

#include "../../include/sfe_dsp.h"

namespace sfe {

constexpr int OCC_MIN_BINS = 8, OCC_MAX_BINS = 4096, OCC_MAX_EMISSIONS = 64;
constexpr int OCC_TILE_LOG2 = 4;                    // a tile of the folds: 16 aligned scan positions
constexpr uint32_t OCC_QNAN = 0x7fc00000u;          // floor and thr of a non-finite row

struct OccParams {
    int n, rank, gap, min_width, n_em, shift;
    float factor, min_level;
};

OCC_HD inline uint32_t occ_bits(float v)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __float_as_uint(v);
#else
    uint32_t b;
    memcpy(&b, &v, sizeof(b));
    return b;
#endif
}

OCC_HD inline float occ_float(uint32_t b)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __uint_as_float(b);
#else
    float v;
    memcpy(&v, &b, sizeof(v));
    return v;
#endif
}

// the total order of step 3: ascending keys are ascending values, -0 below +0
OCC_HD inline uint32_t occ_key(uint32_t bits) { return bits ^ ((bits & 0x80000000u) ? 0xffffffffu : 0x80000000u); }
OCC_HD inline uint32_t occ_unkey(uint32_t key) { return key ^ ((key & 0x80000000u) ? 0x80000000u : 0xffffffffu); }
OCC_HD inline bool occ_finite(uint32_t bits) { return (bits & 0x7f800000u) != 0x7f800000u; }

// step 4: one multiply, then the greater of the two in the order of the keys (neither is a NaN: the row and the parameters are finite)
OCC_HD inline float occ_thr(float factor, float floor, float min_level)
{
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const float t = factor * floor;
    return occ_key(occ_bits(t)) >= occ_key(occ_bits(min_level)) ? t : min_level;
}

// step 7: the fold steps, and whether (v at p) takes the peak from (bv at bp)
OCC_HD inline float occ_sum_step(float acc, float x) { return acc + x; }
OCC_HD inline float occ_mom_step(float acc, int d, float x) { return fmaf((float)d, x, acc); }
OCC_HD inline bool occ_better(float v, int p, float bv, int bp) { return v > bv || (v == bv && p < bp); }

// step 1: the row's own index of scan position p; o is 0 or n / 2
OCC_HD inline int occ_src(int p, int n, int o)
{
    const int k = p + n - o;
    return k >= n ? k - n : k;
}

}  // namespace sfe

// ---- the host's statement of the law (host functions: a device pass parses them and emits nothing)
#include <algorithm>

namespace sfe {

// one emission [lo, hi] of the scan xs, steps 7 and 8
inline void occ_plan_emission(const float *xs, int lo, int hi, int o, sfe_occ_rec *r)
{
    float sum = 0.0f, mom = 0.0f, bv = xs[lo];
    int bp = lo;
    for (int t = lo >> OCC_TILE_LOG2; t <= hi >> OCC_TILE_LOG2; t++) {
        const int a = std::max(lo, t << OCC_TILE_LOG2), b = std::min(hi, (t << OCC_TILE_LOG2) + (1 << OCC_TILE_LOG2) - 1);
        float ps = 0.0f, pm = 0.0f;
        for (int p = a; p <= b; p++) {
            ps = occ_sum_step(ps, xs[p]);
            pm = occ_mom_step(pm, p - lo, xs[p]);
            if (occ_better(xs[p], p, bv, bp)) {
                bv = xs[p];
                bp = p;
            }
        }
        sum = occ_sum_step(sum, ps);
        mom = occ_sum_step(mom, pm);
    }
    r->lo = lo - o;
    r->hi = hi - o;
    r->peak = bp - o;
    r->peak_val = bv;
    r->sum = sum;
    r->moment = mom;
    r->zero[0] = r->zero[1] = 0;
}

// The whole law on one row x[0 .. n): info, rec[0 .. n_em) and mask[0 .. n), each may be null.  The parameters are the
// caller's to check (api_occ.hip: occ_check).
inline void occ_plan_row(const OccParams &P, const float *x, sfe_occ_info *info, sfe_occ_rec *rec, uint8_t *mask)
{
    static_assert(sizeof(sfe_occ_info) == 16 && sizeof(sfe_occ_rec) == 32, "the records' layout is part of the ABI");
    float xs[OCC_MAX_BINS];
    uint32_t key[OCC_MAX_BINS];
    const int n = P.n, o = P.shift ? n / 2 : 0;
    bool bad = false;
    for (int p = 0; p < n; p++) {
        xs[p] = x[occ_src(p, n, o)];
        const uint32_t b = occ_bits(xs[p]);
        bad = bad || !occ_finite(b);
        key[p] = occ_key(b);
    }
    if (rec) memset(rec, 0, sizeof(sfe_occ_rec) * (size_t)P.n_em);
    if (mask) memset(mask, 0, (size_t)n);
    if (bad) {
        if (info) {
            info->floor = info->thr = occ_float(OCC_QNAN);
            info->count = 0;
            info->status = SFE_OCC_NONFINITE;
        }
        return;
    }
    std::nth_element(key, key + P.rank, key + n);
    const float floor = occ_float(occ_unkey(key[P.rank]));
    const float thr = occ_thr(P.factor, floor, P.min_level);
    uint32_t count = 0;
    int lo = -1, last = -1;         // the open run's first occupied position, the last occupied position seen
    auto close_run = [&](int a, int b) {
        if (b - a + 1 < P.min_width) return;
        if (rec && count < (uint32_t)P.n_em) occ_plan_emission(xs, a, b, o, rec + count);
        if (mask)
            for (int p = a; p <= b; p++) mask[occ_src(p, n, o)] = 1;
        count++;
    };
    for (int p = 0; p < n; p++) {
        if (!(xs[p] > thr)) continue;
        if (lo < 0) {
            lo = p;
        } else if (p - last - 1 > P.gap) {
            close_run(lo, last);
            lo = p;
        }
        last = p;
    }
    if (lo >= 0) close_run(lo, last);
    if (info) {
        info->floor = floor;
        info->thr = thr;
        info->count = count;
        info->status = count > (uint32_t)P.n_em ? SFE_OCC_TRUNCATED : 0u;
    }
}

}  // namespace sfe
