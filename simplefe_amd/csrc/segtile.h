// segtile.h -- the LDS of the direct general-rate kernel (polyphase.hip: poly_seg_kernel) and how a reference call -- blksize
// samples -- is dealt to workgroups when it does not fit one.  HOST ONLY (no HIP; the kernel shares the constants and seg_row):
// tests/host/test_seg_split.cpp checks the sizing against every part's real span without a GPU.
//
// A workgroup holds, in this order: up to SEG_MAX_LDS runs of its call (timelaw.h), the taps (U rows + one shifted row of
// seg_row(plen) floats; taps_global: none, they are read from memory) and a tile of the call's samples.  split == 1: the whole
// call and plen samples before it.  split > 1: the call's outputs are dealt in equal runs of output indices to `split`
// workgroups, and each stages the input span ITS outputs reach (seg_part_span).  That span is not max_m / split plus a fixed
// slack: the float32 time law steps by a different amount in every binade, so equal runs of outputs cover unequal runs of
// samples -- the launcher sizes the tile from the largest real span of any part of any call of the launch (seg_tile_plan),
// and the kernel relies on it: it does not clamp.
#pragma once
#include <math.h>
#include <stddef.h>

#include "timelaw.h"

namespace sfe {

constexpr int SEG_MAX_LDS = 96;                          // runs of a call staged in LDS (the rest are read from memory)
constexpr size_t SEG_RUN_BYTES = sizeof(TlSeg);          // one run; polyphase.hip's DevSeg is the same 24 bytes
static_assert(sizeof(TlSeg) == 24, "TlSeg is uploaded as is and read by the kernels as DevSeg / RunLds");
constexpr size_t SEG_LDS_BYTES = 64 * 1024;
constexpr int SEG_MAX_SPLIT = 64;

// >= plen + 1 (the shifted rows read one tap further), a multiple of 4 floats, and never a multiple of 64 floats: a wave's
// lanes read up to U different rows at once (one per phase), and rows a multiple of 256 bytes apart would put the same
// tap of every phase on the same banks -- a U-way conflict on every 16-byte tap read
constexpr int seg_row(int plen) { return ((plen + 4) & ~3) % 64 == 0 ? ((plen + 4) & ~3) + 4 : (plen + 4) & ~3; }

constexpr size_t seg_taps_bytes(int U, int plen) { return (size_t)(U + 1) * seg_row(plen) * 4; }

// LDS of one workgroup whose tile holds `tile` samples of `esz` bytes
constexpr size_t seg_lds_bytes(int U, int plen, int esz, long long tile, bool taps_global)
{
    return SEG_MAX_LDS * SEG_RUN_BYTES + (taps_global ? 0 : seg_taps_bytes(U, plen)) + (size_t)tile * esz;
}

static inline long long seg_floordiv(long long a, int b)      // == polyphase.hip: floordiv
{
    const long long q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

// The tile of part `part` of `split` (split > 1) of one call -- `runs` its n_seg runs, m samples, n_out outputs --, by the
// kernel's own arithmetic (poly_seg_kernel: ka, kb, sample_of, rel0, span): *rel0 its first sample relative to the call's
// first, *n_tile the samples it stages (<= 0 in the out_len-exhausted state when all its outputs lie before the call).  Returns
// false when the part owns no output (the workgroup returns at once).  cursor (optional): a run at or before the part's first
// output's, left at its last output's -- the kernel walks from run 0, which finds the same runs
static inline bool seg_part_span(const TlSeg *runs, int m, int n_out, int U, int plen, int split, int part, long long *rel0,
                                 long long *n_tile, int *cursor = nullptr)
{
    const int ka = (int)((long long)n_out * part / split), kb = (int)((long long)n_out * (part + 1) / split);
    if (ka >= kb) return false;
    int q = cursor ? *cursor : 0;
    auto sample_of = [&](int k) -> long long {
        while (k >= runs[q].k0 + runs[q].count) q++;
        const TlSeg &g = runs[q];
        return seg_floordiv((long long)floor(g.t0 + (double)(k - g.k0) * (double)g.d), U);
    };
    const long long n_first = sample_of(ka), n_last = sample_of(kb - 1) + 1;
    if (cursor) *cursor = q;
    long long r0 = -plen;
    if (part > 0) r0 = n_first - plen;
    long long span = n_last - r0 + 1;
    if (span > m - r0) span = m - r0;
    *rel0 = r0;
    *n_tile = span;
    return true;
}

// The largest tile any part of one call needs at `split` (split == 1: the whole call, m + plen samples)
static inline long long seg_max_span(const TlSeg *runs, int m, int n_out, int U, int plen, int split)
{
    if (split == 1) return (long long)m + plen;
    long long mx = 0;
    int cursor = 0;
    for (int part = 0; part < split; part++) {
        long long rel0, n_tile;
        if (seg_part_span(runs, m, n_out, U, plen, split, part, &rel0, &n_tile, &cursor) && n_tile > mx) mx = n_tile;
    }
    return mx;
}

struct SegTilePlan {
    int    split;           // workgroups per reference call (1 ... SEG_MAX_SPLIT, a power of two)
    int    tile_cap;        // samples a workgroup's tile holds
    int    taps_global;     // the taps stay in memory
    size_t lds_bytes;
};

// Sizes one launch of poly_seg_kernel: max_m the largest call of the launch, max_span(split) the largest tile any part of any of
// its calls needs at that split (seg_max_span over the calls; asked for split > 1 only, each value at most once).  The taps leave
// the LDS only when they are large (> 24 KiB) and a whole call does not fit beside them; the split doubles until the tile fits.
// SFE_ESTATE: no split up to SEG_MAX_SPLIT fits 64 KiB (the caller schedules the outputs on the host).
template <class MaxSpan>
static inline int seg_tile_plan(int U, int plen, int esz, int max_m, MaxSpan max_span, SegTilePlan *out)
{
    long long spans[7] = {(long long)max_m + plen + 1, -1, -1, -1, -1, -1, -1};      // per log2(split)
    auto tile = [&](int split) -> long long {
        int li = 0;
        while ((1 << li) < split) li++;
        if (spans[li] < 0) spans[li] = max_span(split);
        return spans[li];
    };
    auto fits = [&](int split, bool tg) { return seg_lds_bytes(U, plen, esz, tile(split), tg) <= SEG_LDS_BYTES; };
    bool tg = seg_taps_bytes(U, plen) > 24 * 1024 && !fits(1, false);
    int split = 1;
    while (split < SEG_MAX_SPLIT && !fits(split, tg)) split *= 2;
    if (!fits(split, tg) && !tg) {
        tg = true;
        split = 1;
        while (split < SEG_MAX_SPLIT && !fits(split, true)) split *= 2;
    }
    if (!fits(split, tg)) return SFE_ESTATE;
    out->split = split;
    out->tile_cap = (int)tile(split);
    out->taps_global = tg ? 1 : 0;
    out->lds_bytes = seg_lds_bytes(U, plen, esz, tile(split), tg);
    return SFE_OK;
}

}  // namespace sfe
