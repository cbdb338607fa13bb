// rs_plan.h -- the host arithmetic of one resample / decimate process_stream call, before anything is launched: whether the
// step has the closed form, that closed form, and the plan of a general-rate call -- the replay of the float32 time law
// (timelaw.h) reference call by reference call, memoised per start state -- with the two walks over such a plan that the
// launch needs (the direct kernel's tile spans, segtile.h; the per-output schedule of the fallback kernel).  HOST ONLY
// (no HIP, nothing of the library's but timelaw.h and segtile.h): tests/host/test_rs_plan.cpp checks every piece against
// the literal time_law without a GPU.  api_rs.hip is the caller; the chunk type is a template parameter because the
// kernels' SegChunk lives in common.h, which a host program cannot include.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <unordered_map>
#include <vector>

#include "segtile.h"
#include "timelaw.h"

namespace sfe {

// ---- integer-valued steps: the float32 recurrence is exact and has a closed form
// fl(rate * U) is a whole number of upsampled positions (below 1e6: it goes into an int)
static inline bool rs_step_is_integer(float stepf) { return stepf >= 1.0f && stepf == floorf(stepf) && stepf < 1.0e6f; }

// ... and the calls of a handle follow the closed form: no fraction carried, every position of a blksize-sample call exact
// in float32
static inline bool rs_int_step_law(float stepf, const sfe_rs_timestate &ts, int blksize, int U)
{
    return rs_step_is_integer(stepf) && ts.mu == 0.0f && ((double)blksize * U + stepf) < 16777216.0;
}

// One call of n_in samples at the integer step S from state ts: output k at pos0 + k*S, emitted while pos <= n_in*U - 2
// (pos == n_in*U - 1 is the reference's "leftover": it comes out first next call).
struct RsIntCall {
    long long pos0, K;
    sfe_rs_timestate after;
};
static inline RsIntCall rs_int_call(const sfe_rs_timestate &ts, int U, long long n_in, long long S)
{
    RsIntCall c;
    c.pos0 = ts.leftover ? -1 : (long long)ts.pos;
    const long long lim = n_in * U - 2;
    c.K = c.pos0 <= lim ? (lim - c.pos0) / S + 1 : 0;
    const long long next = c.pos0 + c.K * S - n_in * U;
    c.after.leftover = next == -1 ? 1 : 0;
    c.after.pos = (int32_t)next;
    c.after.mu = 0.0f;
    return c;
}

// ---- general rate: the plan of one blksize-sample reference call depends only on the time state the call
// starts in, and that state is a multiple of the float32 grid of the call's LAST binade inside
// [-1, step) -- a few thousand possible values (blksize*U = 16384: 2^-10 apart) -- so plans are
// memoised per start state: a 2^28-sample call replays 65 536 reference calls as table look-ups
// instead of 65 536 x ~40 runs of float arithmetic (36 ms -> ~2 ms on the host), and the run table
// lives on the device across calls (only what is new is uploaded).
struct SegPlanRef {
    int seg_first, n_seg, n_out;
    sfe_rs_timestate after;
    int next = -1;                     // index of the plan for the state this call ends in, once it has been met:
                                       // a stream of full-size calls then walks the plans by index, no hashing
    int max_span[7] = {-1, -1, -1, -1, -1, -1, -1};     // per log2(split): the largest tile a part of this call needs
                                                        // (segtile.h: seg_max_span), once it has been asked for
};
struct RsMemo {
    std::unordered_map<uint64_t, int> index;     // start state -> index into refs
    std::vector<SegPlanRef> refs;
    std::vector<TlSeg> table;           // runs of the memoised calls, in the order they were first met
    float rate = 0.0f;                  // the memo is for one (rate, blksize)
    int m = 0;
    size_t max_segs = (size_t)2 << 20;  // 64 MiB of runs: beyond, calls are planned without the memo
};

static inline uint64_t rs_state_key(const sfe_rs_timestate &st)      // pos >= -1
{
    uint32_t mu_bits;
    memcpy(&mu_bits, &st.mu, 4);
    return ((uint64_t)(uint32_t)(st.pos + 1) << 33) | ((uint64_t)mu_bits << 1) | (uint64_t)(st.leftover ? 1 : 0);
}

// What rs_plan_calls makes of one launch.  Chunk: common.h's SegChunk, or a program's own with the same members.
template <class Chunk>
struct RsPlan {
    std::vector<Chunk> chunks;          // per reference call; seg_first indexes the memo's table with `extra` behind it
    std::vector<int> chunk_ref;         // per call: its memoised plan, -1 for the calls in `extra`
    std::vector<TlSeg> extra;           // runs of calls that are not memoised (the ragged last one)
    size_t n_table = 0;                 // the memo's table when the launch was planned
    size_t K = 0;                       // outputs of the launch
    int max_m = 0;
    // A reference call that runs out of out_len mid-block leaves its time state BEFORE the next call's first sample
    // (pos < -1; SURVEY.md section 5 -- it happens when the float32 recurrence drifts by more outputs than the
    // ceil(n_in / rate) + 2 a call is given, e.g. blksize 16384 x 3 phases at the rate 0.77).  The direct kernel
    // reproduces that state output for output; the transform-domain kernel assigns outputs to blocks by position and
    // does not take such calls.
    bool exhausted = false;             // a call of the launch started in that state
    bool memo_cleared = false;          // the memo was for another (rate, blksize): what the device holds of its table is void
    sfe_rs_timestate after;             // the time state behind the launch
    size_t n_segs() const { return n_table + extra.size(); }
    const TlSeg &seg_at(const RsMemo &memo, size_t i) const { return i < n_table ? memo.table[i] : extra[i - n_table]; }
};

// Replay the float32 recurrence call by call (blksize samples each), as the reference
// object would see the stream -- in closed form: each call becomes a few constant-increment
// runs (timelaw.h) that one workgroup expands on the GPU.  A call's runs are a function of
// the state it starts in; full-size calls are memoised per start state (RsMemo).
template <class Chunk>
static inline RsPlan<Chunk> rs_plan_calls(RsMemo &memo, sfe_rs_timestate st, int U, int blksize, size_t n_in, float rate)
{
    RsPlan<Chunk> p;
    if (memo.rate != rate || memo.m != blksize) {
        memo.index.clear();
        memo.refs.clear();
        memo.table.clear();
        p.memo_cleared = true;
        memo.rate = rate;
        memo.m = blksize;
    }
    std::vector<size_t> extra_chunks;
    p.chunks.reserve(n_in / (size_t)blksize + 1);
    p.chunk_ref.reserve(n_in / (size_t)blksize + 1);
    int prev_ref = -1;          // plan of the previous (memoised) call of this launch: its `next` link is followed / filled in
    for (size_t off = 0; off < n_in; off += (size_t)blksize) {
        const int m = (int)((n_in - off) < (size_t)blksize ? (n_in - off) : (size_t)blksize);
        const int cap = (int)ceilf((float)m / rate) + 2;
        p.exhausted = p.exhausted || st.pos < -1;
        Chunk c;
        c.in_off = (long long)off;
        c.k_first = (long long)p.K;
        c.m = m;
        if (m == blksize && memo.table.size() < memo.max_segs) {
            int idx = prev_ref >= 0 ? memo.refs[(size_t)prev_ref].next : -1;
            if (idx < 0) {
                const uint64_t key = rs_state_key(st);
                auto it = memo.index.find(key);
                if (it == memo.index.end()) {
                    SegPlanRef ref;
                    ref.seg_first = (int)memo.table.size();
                    sfe_rs_timestate st2 = st;
                    ref.n_out = time_law_segments(&st2, U, m, cap, rate, memo.table);
                    ref.n_seg = (int)memo.table.size() - ref.seg_first;
                    ref.after = st2;
                    idx = (int)memo.refs.size();
                    memo.refs.push_back(ref);
                    memo.index.emplace(key, idx);
                } else {
                    idx = it->second;
                }
                if (prev_ref >= 0) memo.refs[(size_t)prev_ref].next = idx;
            }
            const SegPlanRef &ref = memo.refs[(size_t)idx];
            st = ref.after;
            c.seg_first = ref.seg_first;
            c.n_seg = ref.n_seg;
            c.n_out = ref.n_out;
            prev_ref = idx;
            p.chunk_ref.push_back(idx);
        } else {
            prev_ref = -1;
            c.seg_first = (int)p.extra.size();                 // + the table's final size, below
            c.n_out = time_law_segments(&st, U, m, cap, rate, p.extra);
            c.n_seg = (int)p.extra.size() - c.seg_first;
            extra_chunks.push_back(p.chunks.size());
            p.chunk_ref.push_back(-1);
        }
        p.chunks.push_back(c);
        p.K += (size_t)c.n_out;
        p.max_m = m > p.max_m ? m : p.max_m;
    }
    p.n_table = memo.table.size();
    for (size_t ci : extra_chunks) p.chunks[ci].seg_first += (int)p.n_table;
    p.after = st;
    return p;
}

// The direct kernel's tile sizing (segtile.h: seg_tile_plan's max_span): the largest input span any part of any call of
// the launch reaches at `split`.  Per memoised plan and split that span is worked out once (SegPlanRef::max_span); the
// calls outside the memo are walked here.
template <class Chunk>
static inline long long rs_plan_max_span(RsMemo &memo, const RsPlan<Chunk> &p, int U, int plen, int split)
{
    int li = 0;
    while ((1 << li) < split) li++;
    long long mx = 0;
    for (size_t i = 0; i < p.chunks.size(); i++) {
        const Chunk &c = p.chunks[i];
        long long v;
        if (c.n_out <= 0) {
            v = 0;                          // (every workgroup of the call returns at once)
        } else if (p.chunk_ref[i] >= 0) {
            SegPlanRef &ref = memo.refs[(size_t)p.chunk_ref[i]];
            if (ref.max_span[li] < 0)
                ref.max_span[li] = (int)seg_max_span(memo.table.data() + ref.seg_first, c.m, c.n_out, U, plen, split);
            v = ref.max_span[li];
        } else {
            v = seg_max_span(&p.seg_at(memo, (size_t)c.seg_first), c.m, c.n_out, U, plen, split);
        }
        mx = v > mx ? v : mx;
    }
    return mx;
}

// Every output of the launch as the per-output schedule kernel reads it: its upsampled position relative to the launch's
// first sample, and its fraction.  pos and mu are sized to the launch's K outputs.
template <class Chunk>
static inline void rs_plan_expand(const RsMemo &memo, const RsPlan<Chunk> &p, int U, std::vector<long long> &pos, std::vector<float> &mu)
{
    pos.resize(p.K);
    mu.resize(p.K);
    for (const Chunk &c : p.chunks)
        for (int i = 0; i < c.n_seg; i++) {
            const TlSeg &g = p.seg_at(memo, (size_t)c.seg_first + i);
            for (int q = 0; q < g.count; q++) {
                const double t = g.t0 + (double)q * (double)g.d, fl = floor(t);
                pos[(size_t)c.k_first + g.k0 + q] = c.in_off * U + (long long)fl;
                mu[(size_t)c.k_first + g.k0 + q] = (float)(t - fl);
            }
        }
}

}  // namespace sfe
