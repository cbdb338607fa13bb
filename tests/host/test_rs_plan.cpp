// test_rs_plan.cpp -- csrc/rs_plan.h alone, built by a plain host compiler under -fsanitize=address,undefined
// (tests/test_rs_plan_host.py): what a resample / decimate process_stream call works out before it launches.  The oracle
// throughout is the literal time_law (timelaw.h; itself held to the compiled reference by tests/test_host_logic.py), replayed
// reference call by reference call with the out_len the handle gives a call and the state carried -- never the planner.
//   planner     its runs, expanded by rs_plan_expand, are the literal law's (position, mu) sequence bit for bit; so are K, every
//               chunk's n_out / in_off / k_first / m, the out_len-exhausted flag and the end state
//   memo        one launch, launches of one call, launches of three calls: the same stream; a warm memo adds nothing; another
//               rate or blksize clears it; with a small run limit a launch crosses from memoised to un-memoised calls and
//               every chunk's seg_first still names that call's runs
//   span walk   rs_plan_max_span == seg_max_span over each call's own runs, at splits 2, 8, 64, first and cached answer
//   closed form rs_int_call == the literal law on integer steps; the conditions that guard it
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../simplefe_amd/csrc/rs_plan.h"

using namespace sfe;

namespace {

struct Chunk {                  // common.h's SegChunk, member for member
    long long in_off, k_first;
    int m, n_out, seg_first, n_seg;
};
using Plan = RsPlan<Chunk>;

long long g_checks = 0, g_fails = 0;
void expect(int line, bool ok, const char *what)
{
    g_checks++;
    if (ok) return;
    if (++g_fails <= 20) printf("line %d: %s\n", line, what);
}
#define TRUE(x) expect(__LINE__, (x), #x)

bool same_bits(float a, float b) { return memcmp(&a, &b, 4) == 0; }
bool same_state(const sfe_rs_timestate &a, const sfe_rs_timestate &b)
{
    return a.pos == b.pos && same_bits(a.mu, b.mu) && a.leftover == b.leftover;
}
int call_out_len(int m, float rate) { return (int)ceilf((float)m / rate) + 2; }      // what a reference call is given

// ---- the oracle: n_in samples fed to one reference object in blksize-sample calls, by the literal law
struct Literal {
    std::vector<long long> pos;                 // every output's upsampled position, relative to the stream's first sample
    std::vector<float> mu;
    std::vector<int> n_out, m;                  // per call
    std::vector<sfe_rs_timestate> start;        // per call: the state it started in
    bool exhausted = false;                     // a call started before its own first sample (pos < -1)
    sfe_rs_timestate after;
};
Literal literal(sfe_rs_timestate st, int U, int blksize, long long n_in, float rate, long long first = 0)
{
    Literal L;
    for (long long off = 0; off < n_in; off += blksize) {
        const int m = (int)(n_in - off < blksize ? n_in - off : blksize);
        L.exhausted = L.exhausted || st.pos < -1;
        L.start.push_back(st);
        const long long base = (first + off) * U;
        L.n_out.push_back(time_law(&st, U, m, call_out_len(m, rate), rate, [&](int p, float f) {
            L.pos.push_back(base + p);
            L.mu.push_back(f);
        }));
        L.m.push_back(m);
    }
    L.after = st;
    return L;
}

// a launch's plan against the oracle's stretch of the stream that begins at sample `first`, output `k0` and call `call0`
void check_plan(const RsMemo &memo, const Plan &p, const Literal &L, int U, int blksize, long long first = 0, size_t k0 = 0,
                size_t call0 = 0, bool whole = true)
{
    std::vector<long long> pos;
    std::vector<float> mu;
    rs_plan_expand(memo, p, U, pos, mu);
    TRUE(pos.size() == p.K && mu.size() == p.K && k0 + p.K <= L.pos.size() && call0 + p.chunks.size() <= L.n_out.size());
    TRUE(p.chunk_ref.size() == p.chunks.size());
    if (whole) TRUE(p.K == L.pos.size() && p.chunks.size() == L.n_out.size() && p.exhausted == L.exhausted && same_state(p.after, L.after));
    if (k0 + p.K > L.pos.size() || call0 + p.chunks.size() > L.n_out.size()) return;
    bool seq = true;
    for (size_t k = 0; k < p.K; k++) seq = seq && pos[k] + first * U == L.pos[k0 + k] && same_bits(mu[k], L.mu[k0 + k]);
    TRUE(seq);
    size_t K = 0;
    int max_m = 0;
    for (size_t i = 0; i < p.chunks.size(); i++) {
        const Chunk &c = p.chunks[i];
        TRUE(c.in_off == (long long)i * blksize && c.k_first == (long long)K && c.m == L.m[call0 + i] && c.n_out == L.n_out[call0 + i]);
        // the chunk's seg_first names ITS runs: those of one call from the oracle's start state, in the memo's table or behind it
        std::vector<TlSeg> own;
        sfe_rs_timestate st = L.start[call0 + i];
        const int n = time_law_segments(&st, U, c.m, call_out_len(c.m, memo.rate), memo.rate, own);
        bool runs = n == c.n_out && (int)own.size() == c.n_seg && (size_t)c.seg_first + c.n_seg <= p.n_segs();
        for (int q = 0; runs && q < c.n_seg; q++) runs = memcmp(&own[q], &p.seg_at(memo, (size_t)c.seg_first + q), sizeof(TlSeg)) == 0;
        TRUE(runs);
        TRUE(p.chunk_ref[i] >= 0 ? (size_t)c.seg_first + c.n_seg <= p.n_table && memo.refs[p.chunk_ref[i]].seg_first == c.seg_first
                                 : (size_t)c.seg_first >= p.n_table);
        K += (size_t)c.n_out;
        max_m = c.m > max_m ? c.m : max_m;
    }
    TRUE(K == p.K && max_m == p.max_m && p.n_table == memo.table.size());
}

// rs_plan_max_span against seg_max_span over each call's own runs; asked twice (the second answer is the memoised one)
void check_spans(RsMemo &memo, const Plan &p, const Literal &L, int U, size_t call0 = 0)
{
    for (int plen : {8, 32})
        for (int split : {2, 8, 64}) {
            long long want = 0;
            for (size_t i = 0; i < p.chunks.size(); i++) {
                if (L.n_out[call0 + i] <= 0) continue;
                std::vector<TlSeg> own;
                sfe_rs_timestate st = L.start[call0 + i];
                const int m = L.m[call0 + i];
                time_law_segments(&st, U, m, call_out_len(m, memo.rate), memo.rate, own);
                const long long v = seg_max_span(own.data(), m, L.n_out[call0 + i], U, plen, split);
                want = v > want ? v : want;
            }
            // the cache is per plan and split, for ONE plen (a handle has one): clear it between the two
            for (SegPlanRef &ref : memo.refs)
                for (int &v : ref.max_span) v = -1;
            TRUE(rs_plan_max_span(memo, p, U, plen, split) == want);
            TRUE(rs_plan_max_span(memo, p, U, plen, split) == want);
        }
}

long long g_exhausted_cases = 0, g_launches = 0;

void planner_case(int U, int blksize, float rate, long long n_in)
{
    RsMemo memo;
    const sfe_rs_timestate st0 = {0, 0.0f, 0};
    const Literal L = literal(st0, U, blksize, n_in, rate);
    const Plan p = rs_plan_calls<Chunk>(memo, st0, U, blksize, (size_t)n_in, rate);
    g_launches++;
    g_exhausted_cases += L.exhausted;
    TRUE(p.memo_cleared && memo.rate == rate && memo.m == blksize);
    check_plan(memo, p, L, U, blksize);
    check_spans(memo, p, L, U);
}

void test_planner()
{
    const float rates[] = {1.77f, 1.0233f, 3.005f, 0.77f};
    for (int blksize : {64, 128, 1000, 4096})
        for (int U : {1, 2, 3, 5})
            for (float rate : rates) {
                if ((double)rate < 1.0 / U) continue;              // the handle refuses rate < 1 / U
                const long long B = blksize;
                for (long long n_in : {0LL, 1LL, B - 1, 4 * B, 5 * B + 17}) planner_case(U, blksize, rate, n_in);
            }
    // blksize 16384 x 3 phases: at the rate 3.005 (and at the step 3.005, rate 3.005 / 3) the literal law stays clear of the
    // out_len-exhausted state; at the rate 0.77 the second call starts in it -- near position 49152 the float32 grid is 2^-8
    // and the step is rounded down, so a call emits more outputs than ceil(m / rate) + 2 holds
    planner_case(3, 16384, 3.005f, 5 * 16384 + 17);
    planner_case(3, 16384, 3.005f / 3.0f, 5 * 16384 + 17);
    const long long before = g_exhausted_cases;
    planner_case(3, 16384, 0.77f, 5 * 16384 + 17);
    TRUE(g_exhausted_cases == before + 1);
    TRUE(g_exhausted_cases > 0);
}

// one stream through one memo, cut into launches of `calls` reference calls (the last launch: what is left, ragged tail included)
void stream_in_launches(RsMemo &memo, const Literal &L, int U, int blksize, float rate, long long n_in, int calls, bool expect_warm)
{
    const size_t refs0 = memo.refs.size(), table0 = memo.table.size(), index0 = memo.index.size();
    sfe_rs_timestate st = {0, 0.0f, 0};
    size_t k0 = 0, call0 = 0;
    const long long per = (long long)calls * blksize;
    for (long long first = 0; first < n_in; first += per) {
        const long long n = n_in - first < per ? n_in - first : per;
        const Plan p = rs_plan_calls<Chunk>(memo, st, U, blksize, (size_t)n, rate);
        g_launches++;
        TRUE(!p.memo_cleared || (first == 0 && !expect_warm));
        check_plan(memo, p, L, U, blksize, first, k0, call0, false);
        check_spans(memo, p, L, U, call0);
        st = p.after;
        k0 += p.K;
        call0 += p.chunks.size();
    }
    TRUE(k0 == L.pos.size() && call0 == L.n_out.size() && same_state(st, L.after));
    if (expect_warm) TRUE(memo.refs.size() == refs0 && memo.table.size() == table0 && memo.index.size() == index0);
}

void test_memo()
{
    const int U = 3, blksize = 128;
    const float rate = 1.77f;
    const long long n_in = 40LL * blksize + 17;
    const sfe_rs_timestate st0 = {0, 0.0f, 0};
    const Literal L = literal(st0, U, blksize, n_in, rate);
    RsMemo memo;
    stream_in_launches(memo, L, U, blksize, rate, n_in, 1 << 20, false);     // one launch, cold
    TRUE(!memo.refs.empty() && memo.refs.size() == memo.index.size() && memo.refs.size() <= 40);
    stream_in_launches(memo, L, U, blksize, rate, n_in, 1, true);            // launches of one call
    stream_in_launches(memo, L, U, blksize, rate, n_in, 3, true);            // launches of three calls, then the tail
    stream_in_launches(memo, L, U, blksize, rate, n_in, 1 << 20, true);      // the first pass again, warm
    // every call of the stream but the ragged last one is memoised and linked to its successor
    {
        const Plan p = rs_plan_calls<Chunk>(memo, st0, U, blksize, (size_t)n_in, rate);
        bool linked = p.chunk_ref.size() == 41 && p.chunk_ref[40] == -1;
        for (size_t i = 0; linked && i + 1 < 40; i++) linked = p.chunk_ref[i] >= 0 && memo.refs[p.chunk_ref[i]].next == p.chunk_ref[i + 1];
        TRUE(linked);
    }

    // another rate, then another blksize: the memo is cleared and refilled as a fresh one would be
    for (int round = 0; round < 2; round++) {
        const float rate2 = 1.0233f;
        const int blk2 = round ? 64 : blksize;
        const Literal L2 = literal(st0, U, blk2, n_in, rate2);
        RsMemo fresh;
        const Plan pf = rs_plan_calls<Chunk>(fresh, st0, U, blk2, (size_t)n_in, rate2);
        const Plan p2 = rs_plan_calls<Chunk>(memo, st0, U, blk2, (size_t)n_in, rate2);
        TRUE(p2.memo_cleared && memo.rate == rate2 && memo.m == blk2);
        TRUE(memo.refs.size() == fresh.refs.size() && memo.table.size() == fresh.table.size() && memo.index.size() == fresh.index.size());
        TRUE(p2.chunks.size() == pf.chunks.size() && memcmp(p2.chunks.data(), pf.chunks.data(), pf.chunks.size() * sizeof(Chunk)) == 0);
        check_plan(memo, p2, L2, U, blk2);
        const Plan p3 = rs_plan_calls<Chunk>(memo, st0, U, blk2, (size_t)n_in, rate2);
        TRUE(!p3.memo_cleared && memo.refs.size() == fresh.refs.size());
        check_plan(memo, p3, L2, U, blk2);
    }

    // A run limit of 40: the table fills in mid-launch, the calls behind are planned without the memo, their runs lie behind the
    // table and their seg_first is fixed up by the table's final size.  (2^21 runs in the library: no stream of a test gets there.)
    {
        const float rate3 = 1.0233f;
        const Literal L3 = literal(st0, U, blksize, n_in, rate3);
        RsMemo small;
        small.max_segs = 40;
        const Plan p = rs_plan_calls<Chunk>(small, st0, U, blksize, (size_t)n_in, rate3);
        g_launches++;
        size_t first_extra = p.chunk_ref.size();
        for (size_t i = 0; i < p.chunk_ref.size(); i++)
            if (p.chunk_ref[i] < 0 && i < first_extra) first_extra = i;
        bool tail_extra = true;
        for (size_t i = first_extra; i < p.chunk_ref.size(); i++) tail_extra = tail_extra && p.chunk_ref[i] < 0;
        // memoised calls first, then -- in mid-launch, full-size calls among them -- un-memoised ones to the end
        TRUE(first_extra > 0 && first_extra + 2 < p.chunks.size() && p.chunks[first_extra].m == blksize && tail_extra);
        TRUE(small.table.size() >= 40 && p.n_table == small.table.size() && !p.extra.empty());
        TRUE(p.chunks[first_extra].seg_first == (int)p.n_table);
        check_plan(small, p, L3, U, blksize);
        check_spans(small, p, L3, U);
        // the memo is full: the same stream again, call by call, is planned without it and without adding to it
        const size_t table0 = small.table.size();
        stream_in_launches(small, L3, U, blksize, rate3, n_in, 1, true);
        stream_in_launches(small, L3, U, blksize, rate3, n_in, 3, true);
        TRUE(small.table.size() == table0);
    }
}

// ---- integer steps
// rate with fl(rate * U) == S (the handle's stepf)
float rate_for(int S, int U)
{
    float rate = (float)S / (float)U;
    for (int i = 0; i < 4 && rate * (float)U != (float)S; i++) rate = nextafterf(rate, rate * (float)U < (float)S ? INFINITY : 0.0f);
    return rate;
}

void int_case(sfe_rs_timestate st0, int U, int S, int n_in)
{
    const float rate = rate_for(S, U);
    TRUE(rate * (float)U == (float)S);
    TRUE(rs_int_step_law(rate * (float)U, st0, 4096, U));
    const RsIntCall ic = rs_int_call(st0, U, n_in, S);
    sfe_rs_timestate st = st0;
    long long k = 0;
    bool seq = true;
    const int n = time_law(&st, U, n_in, n_in * U + 2, rate, [&](int p, float f) {
        seq = seq && p == ic.pos0 + k * S && f == 0.0f;
        k++;
    });
    TRUE(seq && n == ic.K && k == ic.K);
    TRUE(same_state(st, ic.after));
}

void test_int_step()
{
    const int hl = 64;
    for (int U : {1, 2, 3, 4})
        for (int S : {1, 2, 3, 4, 5, 6, 7, 8, 9, 64})
            for (int n_in : {1, 2, hl, 1000}) {
                for (int pos = -1; pos < S; pos++) int_case({pos, 0.0f, 0}, U, S, n_in);
                int_case({-1, 0.0f, 1}, U, S, n_in);       // a pending leftover output: the law leaves it with pos == -1
            }
    const sfe_rs_timestate z = {0, 0.0f, 0}, frac = {0, 0.25f, 0};
    TRUE(rs_step_is_integer(1.0f) && rs_step_is_integer(64.0f) && rs_step_is_integer(999999.0f));
    TRUE(!rs_step_is_integer(0.0f) && !rs_step_is_integer(0.5f) && !rs_step_is_integer(1.5f) && !rs_step_is_integer(5.3100004f));
    TRUE(!rs_step_is_integer(1.0e6f) && !rs_step_is_integer(3.0e9f) && !rs_step_is_integer(NAN) && !rs_step_is_integer(INFINITY));
    TRUE(rs_int_step_law(8.0f, z, 4096, 1) && rs_int_step_law(5.0f, z, 4096, 3));
    TRUE(!rs_int_step_law(8.0f, frac, 4096, 1));                       // a fraction carried
    TRUE(!rs_int_step_law(5.3100004f, z, 4096, 3));                    // not integral
    TRUE(!rs_int_step_law(1.0e6f, z, 4096, 1));
    TRUE(!rs_int_step_law(8.0f, z, 16777216 / 4 - 2, 4));              // blksize*U + stepf == 2^24
    TRUE(rs_int_step_law(7.0f, z, 16777216 / 4 - 2, 4));               // ... one below it
    TRUE(!rs_int_step_law(8.0f, z, 16777216 / 4, 4));                  // blksize*U alone reaches 2^24
    TRUE(!rs_int_step_law(8.0f, z, 16777208, 1) && rs_int_step_law(7.0f, z, 16777208, 1));
}

}  // namespace

int main()
{
    test_planner();
    test_memo();
    test_int_step();
    if (g_fails) {
        printf("FAIL: %lld of %lld checks\n", g_fails, g_checks);
        return 1;
    }
    printf("rs plan ok: %lld checks over %lld launches, %lld of the planner's cases in the out_len-exhausted state\n", g_checks, g_launches,
           g_exhausted_cases);
    return 0;
}
