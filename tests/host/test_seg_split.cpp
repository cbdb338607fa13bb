// The direct general-rate kernel's tile sizing (simplefe_amd/csrc/segtile.h) against the input every part of a split call
// really reads.  Pure host.  Streams of 8 full reference calls and a ragged last one, the time state carried from call to call
// (timelaw.h: time_law_segments, with the out_len api_rs.hip gives a call), over a grid of blksize, upsample factor, rate, taps
// per phase and sample size.  For every launch the plan either refuses (the caller schedules on the host) or gives a tile that
// holds every part's span in at most 64 KiB.  Independently of seg_part_span, the first and the last output of every part are
// expanded the way the kernel's dot products index the tile (polyphase.hip: dot2) and must read inside it; on a few shapes every
// output is.  Negative control: the rule the launcher used before segtile.h (max_m / split + ceil(rate) + 64 + plen + 2) must
// overflow on a shape where it is known to.
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <iterator>
#include <vector>

#include "../../simplefe_amd/csrc/segtile.h"

using sfe::TlSeg;

namespace {

struct Call {
    int m, n_out;
    bool exhausted;            // started in the reference's out_len-exhausted state (pos < -1)
    std::vector<TlSeg> runs;
};

// the calls of n samples fed to one handle in blksize-sample reference calls (api_rs.hip: rs_process_stream)
std::vector<Call> walk(int U, float rate, int blksize, long long n)
{
    std::vector<Call> calls;
    sfe_rs_timestate st = {0, 0.0f, 0};
    for (long long off = 0; off < n; off += blksize) {
        Call c;
        c.m = (int)(n - off < blksize ? n - off : blksize);
        c.exhausted = st.pos < -1;
        const int cap = (int)ceilf((float)c.m / rate) + 2;
        c.n_out = sfe::time_law_segments(&st, U, c.m, cap, rate, c.runs);
        calls.push_back(std::move(c));
    }
    return calls;
}

long long floordiv(long long a, int b)
{
    const long long q = a / b;
    return (a % b != 0 && a < 0) ? q - 1 : q;
}

// The tile indices output k reads (polyphase.hip: poly_seg_kernel's dot2 with the tile's first sample rel0): x[n - i] for the
// terms of s0 and s1 that lie inside the tile, and x[n + 1] for s1 in the last phase.  Returns false when it reads nothing.
// q: a run at or before output k's (outputs are visited in order)
bool reads_of(const Call &c, int U, int plen, long long rel0, int k, size_t &q, long long *lo, long long *hi)
{
    while (k >= c.runs[q].k0 + c.runs[q].count) q++;
    const TlSeg &g = c.runs[q];
    const long long p = (long long)floor(g.t0 + (double)(k - g.k0) * (double)g.d);
    const long long n = floordiv(p, U);
    const int sh = (int)(p - n * U) + 1 == U;
    const long long reach = n - rel0 + 1;
    const long long L0 = reach < plen ? (reach > 0 ? reach : 0) : plen;
    const long long J1 = reach + sh < plen ? (reach + sh > 0 ? reach + sh : 0) : plen;
    const long long L1 = J1 - (sh && J1 > 0 ? 1 : 0);
    const long long terms = L0 > L1 ? L0 : L1;
    if (terms == 0 && !(sh && J1 > 0)) return false;
    *lo = terms > 0 ? n - rel0 - (terms - 1) : n - rel0 + 1;
    *hi = sh && J1 > 0 ? n - rel0 + 1 : n - rel0;
    return true;
}

long long launch_max_m(const std::vector<Call> &calls, size_t first, size_t last)
{
    long long mx = 0;
    for (size_t i = first; i < last; i++) mx = calls[i].m > mx ? calls[i].m : mx;
    return mx;
}

struct Stats {
    long long launches = 0, refused = 0, taps_global = 0, exhausted_calls = 0, parts = 0, outputs_expanded = 0;
    int max_split = 0;
};

// One launch of poly_seg_kernel over calls [first, last): plan it with segtile.h and check every part.  Returns false (and
// prints) on a part whose reads leave its tile or a tile beyond the LDS.  every_output: expand every output, not the ends.
bool check_launch(const std::vector<Call> &calls, size_t first, size_t last, int U, int plen, int esz, bool every_output,
                  const char *what, Stats &S)
{
    const int max_m = (int)launch_max_m(calls, first, last);
    auto max_span = [&](int split) -> long long {
        long long mx = 0;
        for (size_t i = first; i < last; i++) {
            if (calls[i].n_out <= 0) continue;
            const long long v = sfe::seg_max_span(calls[i].runs.data(), calls[i].m, calls[i].n_out, U, plen, split);
            mx = v > mx ? v : mx;
        }
        return mx;
    };
    sfe::SegTilePlan tp;
    S.launches++;
    if (sfe::seg_tile_plan(U, plen, esz, max_m, max_span, &tp) != SFE_OK) {
        S.refused++;
        return true;
    }
    S.taps_global += tp.taps_global;
    S.max_split = tp.split > S.max_split ? tp.split : S.max_split;
    if (tp.lds_bytes > sfe::SEG_LDS_BYTES || tp.lds_bytes != sfe::seg_lds_bytes(U, plen, esz, tp.tile_cap, tp.taps_global != 0) ||
        tp.split < 1 || tp.split > sfe::SEG_MAX_SPLIT) {
        printf("FAIL %s: plan split %d tile_cap %d lds %zu\n", what, tp.split, tp.tile_cap, tp.lds_bytes);
        return false;
    }
    for (size_t ci = first; ci < last; ci++) {
        const Call &c = calls[ci];
        if (c.n_out <= 0) continue;
        size_t q = 0;                            // (parts, and their outputs, are visited in order)
        for (int part = 0; part < tp.split; part++) {
            long long rel0 = -plen, n_tile = (long long)c.m + plen;
            int ka = 0, kb = c.n_out;
            if (tp.split > 1) {
                if (!sfe::seg_part_span(c.runs.data(), c.m, c.n_out, U, plen, tp.split, part, &rel0, &n_tile)) continue;
                ka = (int)((long long)c.n_out * part / tp.split);
                kb = (int)((long long)c.n_out * (part + 1) / tp.split);
            }
            S.parts++;
            if (n_tile > tp.tile_cap) {          // (n_tile <= 0: a part of a call in the exhausted state whose outputs lie before the tile, reading nothing)
                printf("FAIL %s: call %zu part %d of %d: span %lld > tile_cap %d\n", what, ci - first, part, tp.split, n_tile, tp.tile_cap);
                return false;
            }
            for (int k = ka; k < kb; k = (every_output || k >= kb - 2) ? k + 1 : kb - 1) {
                long long lo, hi;
                S.outputs_expanded++;
                if (reads_of(c, U, plen, rel0, k, q, &lo, &hi) && (lo < 0 || hi >= n_tile)) {
                    printf("FAIL %s: call %zu part %d of %d output %d reads tile[%lld .. %lld], the part stages %lld\n", what,
                           ci - first, part, tp.split, k, lo, hi, n_tile);
                    return false;
                }
            }
        }
    }
    return true;
}

// The launcher's rule before segtile.h: a part's tile = ceil(max_m / split) + ceil(rate) + 64 + plen + 2.  Returns the worst
// amount by which a part's real span exceeded it (<= 0: none did), the split and tile_cap it chose, and where.
long long old_rule_excess(const std::vector<Call> &calls, int U, int plen, int esz, float rate, int *split_out, int *cap_out,
                          int *call_out, int *part_out)
{
    const int max_m = (int)launch_max_m(calls, 0, calls.size());
    const long long slack = (long long)ceilf(rate) + 64;
    const size_t taps_b = sfe::seg_taps_bytes(U, plen);
    auto tile = [&](int split) -> long long { return split == 1 ? (long long)max_m + plen + 1 : (max_m + split - 1) / split + slack + plen + 2; };
    auto need = [&](int split, bool tg) { return sfe::SEG_MAX_LDS * sfe::SEG_RUN_BYTES + (tg ? 0 : taps_b) + (size_t)tile(split) * esz; };
    bool tg = taps_b > 24 * 1024 && need(1, false) > sfe::SEG_LDS_BYTES;
    int split = 1;
    while (split < 64 && need(split, tg) > sfe::SEG_LDS_BYTES) split *= 2;
    if (need(split, tg) > sfe::SEG_LDS_BYTES && !tg) {
        tg = true;
        split = 1;
        while (split < 64 && need(split, true) > sfe::SEG_LDS_BYTES) split *= 2;
    }
    *split_out = split;
    *cap_out = (int)tile(split);
    long long worst = need(split, tg) > sfe::SEG_LDS_BYTES ? -1 : 0;      // (-1: refused)
    if (worst < 0 || split == 1) return worst;
    for (size_t ci = 0; ci < calls.size(); ci++)
        for (int part = 0, cursor = 0; part < split; part++) {
            long long rel0, n_tile;
            if (!sfe::seg_part_span(calls[ci].runs.data(), calls[ci].m, calls[ci].n_out, U, plen, split, part, &rel0, &n_tile, &cursor)) continue;
            if (n_tile - *cap_out > worst) {
                worst = n_tile - *cap_out;
                *call_out = (int)ci;
                *part_out = part;
            }
        }
    return worst;
}

}  // namespace

int main()
{
    const int blksizes[] = {4096, 8192, 65536, 131072, 262144, 393216, 524288, 786432, 1048576};
    const int Us[] = {1, 2, 3, 7, 16, 31, 32};
    const float rates[] = {1.0233f, 1.77f, 0.77f, 1.3f, 3.3f, 2.5f, 1.0000001f, 0.50000006f, 10.52f};
    const int plens[] = {4, 11, 32, 127};
    // (U, taps per phase): every U of the grid with every plen, and two filters whose taps exceed 24 KiB -- (U + 1) seg_row(plen)
    // floats -- and leave the LDS when a whole call does not fit beside them
    struct Shape { int U; std::vector<int> plens; };
    std::vector<Shape> shapes;
    for (int U : Us) shapes.push_back({U, std::vector<int>(std::begin(plens), std::end(plens))});
    shapes.push_back({64, {127}});
    shapes.push_back({32, {255}});
    Stats S;
    int old_overflows = 0;
    for (int B : blksizes)
        for (float rate : rates)
            for (const Shape &sh : shapes) {
                if ((double)rate < 1.0 / sh.U) continue;                    // the reference refuses rate < 1 / U (api_rs.hip too)
                const long long n = 8LL * B + B / 3 + 7;                   // 8 full calls and a ragged one
                const std::vector<Call> calls = walk(sh.U, rate, B, n);
                for (const Call &c : calls) S.exhausted_calls += c.exhausted;
                for (int plen : sh.plens)
                    for (int esz : {4, 8}) {
                        char what[160];
                        snprintf(what, sizeof what, "%s blksize %d U %d rate %.9g plen %d", esz == 8 ? "complex" : "real", B, sh.U, rate, plen);
                        if (!check_launch(calls, 0, calls.size(), sh.U, plen, esz, false, what, S)) return 1;
                        int split, cap, call = -1, part = -1;
                        if (old_rule_excess(calls, sh.U, plen, esz, rate, &split, &cap, &call, &part) > 0) old_overflows++;
                    }
            }
    if (S.exhausted_calls == 0 || S.taps_global == 0 || S.refused == 0 || S.max_split != sfe::SEG_MAX_SPLIT) {
        printf("FAIL coverage: %lld exhausted calls, %lld taps-global plans, %lld refused, largest split %d\n", S.exhausted_calls,
               S.taps_global, S.refused, S.max_split);
        return 1;
    }

    // Shapes the old rule overflows on, plen 32 and 8 (tests/test_gpu_parity.py runs them on the GPU), the whole stream as
    // one launch (plen 32: every output of every part expanded) and each call as a launch of its own (a stream fed call by call)
    struct Row { bool cplx; int B, U; float rate; };
    const Row rows[] = {{true, 393216, 3, 1.0233f}, {true, 393216, 7, 0.77f}, {true, 393216, 2, 0.77f},
                        {true, 393216, 16, 0.77f}, {false, 393216, 3, 1.0233f}, {false, 393216, 7, 1.77f}, {false, 524288, 3, 1.0233f},
                        {true, 524288, 3, 1.0233f}};
    for (const Row &rw : rows)
        for (int plen : {32, 8}) {
            const long long n = 5LL * rw.B + rw.B / 3;               // tests/test_gpu_parity.py: the stream of the GPU test
            const std::vector<Call> calls = walk(rw.U, rw.rate, rw.B, n);
            char what[160];
            snprintf(what, sizeof what, "%s blksize %d U %d rate %.9g plen %d", rw.cplx ? "complex" : "real", rw.B, rw.U, rw.rate, plen);
            int osplit, ocap, ocall = -1, opart = -1;
            const long long over = old_rule_excess(calls, rw.U, plen, rw.cplx ? 8 : 4, rw.rate, &osplit, &ocap, &ocall, &opart);
            if ((over > 0) != !(rw.cplx && rw.B == 524288)) {          // (that one the old rule refused as well)
                printf("FAIL %s: the old rule (split %d, tile_cap %d) should overflow here: worst part over by %lld\n", what, osplit,
                       ocap, over);
                return 1;
            }
            const long long refused0 = S.refused;
            if (!check_launch(calls, 0, calls.size(), rw.U, plen, rw.cplx ? 8 : 4, plen == 32, what, S)) return 1;
            const bool refused = S.refused > refused0;
            // a complex call of 524288 samples needs more than 64 KiB at any split: the plan must refuse; every other row must not
            if (refused != (rw.cplx && rw.B == 524288)) {
                printf("FAIL %s: plan %s\n", what, refused ? "refused" : "accepted");
                return 1;
            }
            for (size_t i = 0; i < calls.size(); i++) {
                if (calls[i].exhausted) {
                    printf("FAIL %s: call %zu starts in the out_len-exhausted state (the GPU test's oracle cannot follow it)\n", what, i);
                    return 1;
                }
                if (!check_launch(calls, i, i + 1, rw.U, plen, rw.cplx ? 8 : 4, false, what, S)) return 1;
            }
        }

    // negative control: the old rule on the first of those shapes (complex, blksize 393216, U 3, rate 1.0233, plen 32; 4 calls)
    {
        const std::vector<Call> calls = walk(3, 1.0233f, 393216, 4LL * 393216);
        int split, cap, call = -1, part = -1;
        const long long over = old_rule_excess(calls, 3, 32, 8, 1.0233f, &split, &cap, &call, &part);
        printf("old rule, complex blksize 393216 U 3 rate 1.0233 plen 32: split %d tile_cap %d, worst part over by %lld (call %d, part %d)\n",
               split, cap, over, call, part);
        if (split != 64 || cap != 6244 || over <= 0) {
            printf("FAIL negative control: the old rule should overflow here\n");
            return 1;
        }
    }
    printf("segsplit ok: %lld launches (%lld refused, %lld with the taps in memory, split up to %d), %lld parts, %lld outputs "
           "expanded, %lld calls in the out_len-exhausted state; the old rule overflowed on %d of them\n",
           S.launches, S.refused, S.taps_global, S.max_split, S.parts, S.outputs_expanded, S.exhausted_calls, old_overflows);
    return 0;
}
