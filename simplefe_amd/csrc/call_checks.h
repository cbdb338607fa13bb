// call_checks.h -- the argument checks a process_stream makes before it launches anything: what stands between a caller's
// bad stride and an out-of-bounds kernel.  The pieces every block uses (Span, span_bytes, refuse_*), the rules of the burst
// chain's windows and frames (check_starts, check_place), one check per family of blocks: rows (vit, reed, ldpc, crc), windows
// (burst, ofdm), frames (mod, ofdmmod), streams (chan, ddc, psd, iir, polar, beam, cov), channels (fir, fir_calibrate, rs),
// and the byte ranges of the four entry points that fit no family (combine, corr, mvdr, eig).  Every byte range comes from span_bytes, so a stride that would wrap
// one is refused, never multiplied out.  HOST CODE ONLY, plain C++17 and no HIP: block.h includes it, and
// tests/host/test_call_checks.cpp compiles it alone.  `who` is the message prefix ("vit_process_stream") throughout; what
// else differs between the blocks of a family -- their nouns -- comes in as words, never as a format.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <initializer_list>

#include "../../include/sfe_dsp.h"

namespace sfe {

void set_error(const char *fmt, ...);      // api.hip

// [a, a + an) and [b, b + bn) share a byte
inline bool ranges_overlap(const void *a, size_t an, const void *b, size_t bn)
{
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
    return an && bn && pa < pb + bn && pb < pa + an;
}

inline int refuse_2_31(const char *who, size_t n_in)       // the kernels index a stream's samples in 32 bits
{
    if (n_in < ((size_t)1 << 31)) return SFE_OK;
    set_error("%s: n_in = %zu must be below 2^31 per call", who, n_in);
    return SFE_EINVAL;
}

inline int refuse_null(const char *who, std::initializer_list<const void *> bufs)
{
    for (const void *b : bufs)
        if (!b) {
            set_error("%s: null buffer", who);
            return SFE_EINVAL;
        }
    return SFE_OK;
}

// a buffer of `bytes` bytes whose element is `align` bytes (a power of two)
struct Span {
    const void *p;
    size_t bytes, align;
};
inline int refuse_misaligned(const char *who, const char *elements, std::initializer_list<Span> bufs)   // `elements`: for the message
{
    for (const Span &b : bufs)
        if (reinterpret_cast<uintptr_t>(b.p) & (b.align - 1)) {
            set_error("%s: buffers must be aligned to their element (%s)", who, elements);
            return SFE_EINVAL;
        }
    return SFE_OK;
}
// an output of no bytes (a null optional one, a call that completes no row) overlaps nothing
inline int refuse_overlap(const char *who, Span in, std::initializer_list<Span> outs)
{
    for (const Span &o : outs)
        if (ranges_overlap(in.p, in.bytes, o.p, o.bytes)) {
            set_error("%s: input and output ranges overlap (in-place operation is not supported)", who);
            return SFE_EINVAL;
        }
    return SFE_OK;
}
// every pair of a call's outputs
inline int refuse_outputs_overlap(const char *who, std::initializer_list<Span> outs)
{
    for (const Span *a = outs.begin(); a != outs.end(); a++)
        for (const Span *b = a + 1; b != outs.end(); b++)
            if (ranges_overlap(a->p, a->bytes, b->p, b->bytes)) {
                set_error("%s: the output ranges overlap one another", who);
                return SFE_EINVAL;
            }
    return SFE_OK;
}

// bytes = (rows_less_1 * stride + tail) * elem, false where that is not below 2^62
inline bool span_bytes(size_t rows_less_1, size_t stride, size_t tail, size_t elem, size_t *bytes)
{
    size_t v;
    if (__builtin_mul_overflow(rows_less_1, stride, &v) || __builtin_add_overflow(v, tail, &v) || __builtin_mul_overflow(v, elem, &v) ||
        v >= ((size_t)1 << 62))
        return false;
    *bytes = v;
    return true;
}

inline int refuse_2_62(const char *who)      // where a span_bytes failed
{
    set_error("%s: the strides take a byte range to 2^62", who);
    return SFE_EINVAL;
}

// ---- windows cut from a stream (burst, ofdm; their plans too).  o = start_base + b start_step + idx, and what a kernel
// steps back from it, must not leave int64 for any b < n_bursts (at least 1) and any uint32 idx: the sum is linear in b, so
// its two ends decide.
inline int check_starts(const char *who, int64_t start_base, int64_t start_step, size_t n_bursts)
{
    const __int128 room = ((__int128)1 << 63) - ((__int128)1 << 33);
    const __int128 last = (__int128)start_base + (__int128)(n_bursts - 1) * start_step;
    if (start_base < -room || start_base > room || last < -room || last > room) {
        set_error("%s: start_base + b * start_step must stay within +-(2^63 - 2^33) for every burst", who);
        return SFE_EINVAL;
    }
    return SFE_OK;
}

// S streams of n_in samples lie in_stride apart (the windows family, and fsk's demodulator, whose outputs fit no family);
// one stream's stride is not looked at
inline int refuse_short_streams(const char *who, size_t S, size_t in_stride, size_t n_in)
{
    if (S > 1 && in_stride < n_in) {
        set_error("%s: in_stride %zu < n_in %zu with %d streams", who, in_stride, n_in, (int)S);
        return SFE_EINVAL;
    }
    return SFE_OK;
}

// ---- frames of F samples laid into a stream of n_out (mod, ofdmmod; their plans too): where they lie.  even_starts: a
// frame starts on a 5-byte group of the TX10 wire format.
inline int check_place(const char *who, int F, bool tx10, bool even_starts, size_t n_bursts, int64_t start_base, int64_t start_step,
                       size_t n_out)
{
    if (n_out >= ((size_t)1 << 31) || n_bursts >= ((size_t)1 << 31)) {
        set_error("%s: n_out = %zu and n_bursts = %zu must be below 2^31", who, n_out, n_bursts);
        return SFE_EINVAL;
    }
    if (tx10 && (n_out & 1)) {
        set_error("%s: n_out = %zu must be even with SFE_FMT_TX10 (whole 5-byte groups)", who, n_out);
        return SFE_EINVAL;
    }
    if (n_bursts == 0) return SFE_OK;
    if (start_base < 0) {
        set_error("%s: start_base = %lld must not be negative", who, (long long)start_base);
        return SFE_EINVAL;
    }
    if (n_bursts > 1 && start_step < F) {
        set_error("%s: start_step = %lld is below the frame's F = %d samples (frames must not overlap)", who, (long long)start_step, F);
        return SFE_EINVAL;
    }
    if (even_starts && ((start_base & 1) || (n_bursts > 1 && (start_step & 1)))) {
        set_error("%s: start_base = %lld and start_step = %lld must be even with SFE_FMT_TX10 (a frame starts on a 5-byte group)", who,
                  (long long)start_base, (long long)start_step);
        return SFE_EINVAL;
    }
    const __int128 end = (__int128)start_base + (__int128)(n_bursts - 1) * (n_bursts > 1 ? start_step : 0) + F;
    if (end > (__int128)n_out) {
        set_error("%s: the last frame ends behind the stream's n_out = %zu samples", who, n_out);
        return SFE_EINVAL;
    }
    return SFE_OK;
}

// ==== the families.  Each returns SFE_OK with *go = false where the call has nothing to do.

// ---- rows: a codec that reads one row of `in_row` elements of `esz` bytes and writes one of `out_row` bytes per item, with
// an optional status in, record (rec_bytes a row) and status out.  The SFE_ERANGE sentence reads "in_stride S < the R
// <in_row>, or out_stride S < <out_lead>R<out_tail>".  out_optional (crc's check): d_out may be null like the record and the
// status -- an output of no bytes, whose stride is not looked at.
struct RowNouns {
    const char *count;                  // "n_bursts"
    const char *in_row;                 // "elements of a burst's row"
    const char *out_lead, *out_tail;    // "ceil(n_info / 8) = ", ""
    const char *elements;               // refuse_misaligned's
    size_t rec_bytes;
};
inline int check_rows(const char *who, const RowNouns &nn, size_t n, const void *d_in, size_t in_stride, size_t in_row, size_t esz,
                      const void *d_status_in, const void *d_out, size_t out_stride, size_t out_row, const void *d_rec, const void *d_status,
                      bool *go, bool out_optional = false)
{
    *go = false;
    if (n >= ((size_t)1 << 31)) {
        set_error("%s: %s = %zu must be below 2^31 per call", who, nn.count, n);
        return SFE_EINVAL;
    }
    if (n == 0) return SFE_OK;
    int rc = out_optional ? refuse_null(who, {d_in}) : refuse_null(who, {d_in, d_out});
    if (rc != SFE_OK) return rc;
    if (in_stride < in_row || (d_out && out_stride < out_row)) {
        set_error("%s: in_stride %zu < the %zu %s, or out_stride %zu < %s%zu%s", who, in_stride, in_row, nn.in_row, out_stride, nn.out_lead,
                  out_row, nn.out_tail);
        return SFE_ERANGE;
    }
    size_t in_b = 0, ou_b = 0;
    if (!span_bytes(n - 1, in_stride, in_row, esz, &in_b) || (d_out && !span_bytes(n - 1, out_stride, out_row, 1, &ou_b))) {
        set_error("%s: a stride is so large that its buffer's byte range reaches 2^62", who);
        return SFE_EINVAL;
    }
    const Span in{d_in, in_b, esz}, si{d_status_in, d_status_in ? n * 4 : 0, 4}, ou{d_out, ou_b, 1};
    const Span re{d_rec, d_rec ? n * nn.rec_bytes : 0, 4}, st{d_status, d_status ? n * 4 : 0, 4};
    if ((rc = refuse_misaligned(who, nn.elements, {in, si, re, st})) != SFE_OK || (rc = refuse_overlap(who, in, {ou, re, st})) != SFE_OK ||
        (rc = refuse_overlap(who, si, {ou, re, st})) != SFE_OK || (rc = refuse_outputs_overlap(who, {ou, re, st})) != SFE_OK)
        return rc;
    *go = true;
    return SFE_OK;
}

// ---- typed rows (qam): the rows family where every buffer has an element of its own -- per item one row of `in_row`
// elements of isz bytes, where d_side is given one row of `side_row` elements of ssz bytes beside it, and one row of `out_row`
// elements of osz bytes out; the strides count elements.  An element of one byte needs no alignment.  The SFE_ERANGE
// sentence reads "in_stride S < the R <in_row>, <side_name> S < the R <side_row>, or out_stride S < the R <out_row>".
struct TypedRowNouns {
    const char *count;                  // "n_rows"
    const char *in_row, *side_name, *side_row, *out_row;    // "cf32 of a row", "csi_stride", "cf32 of a csi row", "floats of a row"
    const char *elements;               // refuse_misaligned's
};
inline int check_typed_rows(const char *who, const TypedRowNouns &nn, size_t n, const void *d_in, size_t in_stride, size_t in_row, size_t isz,
                            const void *d_side, size_t side_stride, size_t side_row, size_t ssz, const void *d_out, size_t out_stride,
                            size_t out_row, size_t osz, bool *go)
{
    *go = false;
    if (n >= ((size_t)1 << 31)) {
        set_error("%s: %s = %zu must be below 2^31 per call", who, nn.count, n);
        return SFE_EINVAL;
    }
    if (n == 0) return SFE_OK;
    int rc = refuse_null(who, {d_in, d_out});
    if (rc != SFE_OK) return rc;
    if (in_stride < in_row || (d_side && side_stride < side_row) || out_stride < out_row) {
        set_error("%s: in_stride %zu < the %zu %s, %s %zu < the %zu %s, or out_stride %zu < the %zu %s", who, in_stride, in_row, nn.in_row,
                  nn.side_name, side_stride, d_side ? side_row : (size_t)0, nn.side_row, out_stride, out_row, nn.out_row);
        return SFE_ERANGE;
    }
    size_t in_b = 0, si_b = 0, ou_b = 0;
    if (!span_bytes(n - 1, in_stride, in_row, isz, &in_b) || (d_side && !span_bytes(n - 1, side_stride, side_row, ssz, &si_b)) ||
        !span_bytes(n - 1, out_stride, out_row, osz, &ou_b))
        return refuse_2_62(who);
    const Span in{d_in, in_b, isz}, si{d_side, si_b, ssz}, ou{d_out, ou_b, osz};
    if ((rc = refuse_misaligned(who, nn.elements, {in, si, ou})) != SFE_OK || (rc = refuse_overlap(who, in, {ou})) != SFE_OK ||
        (rc = refuse_overlap(who, si, {ou})) != SFE_OK)
        return rc;
    *go = true;
    return SFE_OK;
}

// ---- windows: a receiver that cuts n_bursts windows from each of S streams of n_in samples (isz bytes each) at indices and
// behind gates that are optional, and writes a row of `row` cf32 (`row_name`, for the message) per window, with an optional
// row of chan_row cf32 (ofdm's channel; d_chan null elsewhere), a record of rec_floats and a status.
inline int check_windows(const char *who, const char *row_name, size_t S, size_t isz, const void *d_in, size_t n_in, size_t in_stride,
                         const void *d_idx, size_t idx_stride, const void *d_gate, size_t gate_stride, size_t n_bursts, int64_t start_base,
                         int64_t start_step, const void *d_out, size_t out_stride, size_t row, const void *d_chan, size_t chan_row,
                         const void *d_rec, size_t rec_floats, const void *d_status, size_t status_stride, bool *go)
{
    *go = false;
    int rc = refuse_2_31(who, n_in);
    if (rc != SFE_OK) return rc;
    if (n_bursts >= ((size_t)1 << 31) / S) {
        set_error("%s: n_streams * n_bursts = %zu * %zu must be below 2^31 per call", who, S, n_bursts);
        return SFE_EINVAL;
    }
    if (n_bursts == 0) return SFE_OK;
    if ((rc = refuse_null(who, {d_in, d_out})) != SFE_OK) return rc;
    if (out_stride < row || (d_status && status_stride < n_bursts)) {
        set_error("%s: out_stride %zu < %s = %zu or status_stride %zu < n_bursts = %zu", who, out_stride, row_name, row, status_stride, n_bursts);
        return SFE_ERANGE;
    }
    if ((rc = refuse_short_streams(who, S, in_stride, n_in)) != SFE_OK) return rc;
    if ((rc = check_starts(who, start_base, start_step, n_bursts)) != SFE_OK) return rc;
    const size_t rows = S * n_bursts;
    size_t in_b = 0, ix_b = 0, ga_b = 0, ou_b = 0, st_b = 0;
    if (!span_bytes(S - 1, in_stride, n_in, isz, &in_b) || (d_idx && !span_bytes(S - 1, idx_stride, n_bursts, 4, &ix_b)) ||
        (d_gate && !span_bytes(S - 1, gate_stride, n_bursts, 4, &ga_b)) || !span_bytes(rows - 1, out_stride, row, 8, &ou_b) ||
        (d_status && !span_bytes(S - 1, status_stride, n_bursts, 4, &st_b))) {
        set_error("%s: a stride is so large that its buffer's byte range reaches 2^62", who);
        return SFE_EINVAL;
    }
    const Span in{d_in, in_b, isz}, ix{d_idx, ix_b, 4}, ga{d_gate, ga_b, 4}, ou{d_out, ou_b, 8}, ch{d_chan, d_chan ? rows * chan_row * 8 : 0, 8};
    const Span re{d_rec, d_rec ? rows * rec_floats * 4 : 0, 4}, st{d_status, st_b, 4};
    if ((rc = refuse_misaligned(who, "cf32 8 B, u8 (I,Q) pairs 2 B, indices, gates, records and statuses 4 B", {in, ix, ga, ou, ch, re, st})) != SFE_OK ||
        (rc = refuse_overlap(who, in, {ou, ch, re, st})) != SFE_OK || (rc = refuse_overlap(who, ix, {ou, ch, re, st})) != SFE_OK ||
        (rc = refuse_overlap(who, ga, {ou, ch, re, st})) != SFE_OK || (rc = refuse_outputs_overlap(who, {ou, ch, re, st})) != SFE_OK)
        return rc;
    *go = true;
    return SFE_OK;
}

// ---- frames: a transmitter that reads a row of `in_row` elements of `ie` bytes per burst and lays its frame of F samples
// into a stream of n_out: cf32, or TX10 groups of 5 bytes per 2 samples.  The SFE_ERANGE sentence reads "in_stride S <
// <row_lead>R<row_tail>"; `range_of` names the input in the 2^62 sentence ("payloads'").
struct FrameNouns {
    const char *row_lead, *row_tail;    // "ceil(n_info / 8) = ", ""
    const char *range_of;
    const char *elements;               // refuse_misaligned's
};
inline int check_frames(const char *who, const FrameNouns &nn, int F, bool tx10, bool even_starts, const void *d_in, size_t in_stride,
                        size_t in_row, size_t ie, size_t n_bursts, int64_t start_base, int64_t start_step, const void *d_out, size_t n_out,
                        bool *go)
{
    *go = false;
    int rc = check_place(who, F, tx10, even_starts, n_bursts, start_base, start_step, n_out);
    if (rc != SFE_OK) return rc;
    if (n_out == 0) return SFE_OK;
    if ((rc = refuse_null(who, {d_out})) != SFE_OK || (n_bursts && (rc = refuse_null(who, {d_in})) != SFE_OK)) return rc;
    if (n_bursts && in_stride < in_row) {
        set_error("%s: in_stride %zu < %s%zu%s", who, in_stride, nn.row_lead, in_row, nn.row_tail);
        return SFE_ERANGE;
    }
    size_t in_b = 0;
    if (n_bursts && !span_bytes(n_bursts - 1, in_stride, in_row, ie, &in_b)) {
        set_error("%s: in_stride is so large that the %s byte range reaches 2^62", who, nn.range_of);
        return SFE_EINVAL;
    }
    const Span in{d_in, in_b, ie}, ou{d_out, tx10 ? n_out / 2 * 5 : n_out * 8, tx10 ? (size_t)1 : (size_t)8};
    if ((rc = refuse_misaligned(who, nn.elements, {in, ou})) != SFE_OK || (rc = refuse_overlap(who, in, {ou})) != SFE_OK) return rc;
    *go = true;
    return SFE_OK;
}

// ---- streams: a block that reads in_rows rows of n_in samples (isz bytes each) and writes out_rows rows of `need` elements
// (osz bytes each): chan, ddc, psd, iir, polar, beam, cov, after the block's own granule rule and ahead of its capture refusal.
// The SFE_ERANGE sentence reads "out_stride S < <need>N".  A call that writes nothing (psd and cov complete no row: need = 0)
// has an output of no bytes.
struct StreamNouns {
    const char *need;                   // "n_out ", "n_rows * n_fft = "
    const char *elements;               // refuse_misaligned's
    bool below_2_31;                    // the kernels index n_in in 32 bits (not chan's)
    bool name_streams;                  // the rows are the handle's streams: one row's in_stride is not looked at, and the sentence names them
};
inline int check_streams(const char *who, const StreamNouns &nn, const void *d_in, size_t n_in, size_t in_stride, size_t in_rows, size_t isz,
                         const void *d_out, size_t out_stride, size_t need, size_t out_rows, size_t osz, bool *go)
{
    *go = false;
    int rc = nn.below_2_31 ? refuse_2_31(who, n_in) : SFE_OK;
    if (rc != SFE_OK || n_in == 0) return rc;
    if ((rc = refuse_null(who, {d_in, d_out})) != SFE_OK) return rc;
    if (out_stride < need) {
        set_error("%s: out_stride %zu < %s%zu", who, out_stride, nn.need, need);
        return SFE_ERANGE;
    }
    if (in_stride < n_in && (in_rows > 1 || !nn.name_streams)) {
        if (nn.name_streams) set_error("%s: in_stride %zu < n_in %zu with %d streams", who, in_stride, n_in, (int)in_rows);
        else set_error("%s: in_stride %zu < n_in %zu", who, in_stride, n_in);
        return SFE_EINVAL;
    }
    size_t in_b = 0, out_b = 0;
    if (!span_bytes(in_rows - 1, in_stride, n_in, isz, &in_b) || (need && !span_bytes(out_rows - 1, out_stride, need, osz, &out_b)))
        return refuse_2_62(who);
    const Span in{d_in, in_b, isz}, out{d_out, out_b, osz};
    if ((rc = refuse_misaligned(who, nn.elements, {in, out})) != SFE_OK || (rc = refuse_overlap(who, in, {out})) != SFE_OK) return rc;
    *go = true;
    return SFE_OK;
}

// ---- channels: the FIR and resample / decimate handles read n_channels rows of n elements (isz bytes each) and write
// n_channels rows of up to `cap` elements of osz bytes (FIR: cap = n), or, tx10, of the 5-byte groups that hold 4 floats
// each: fir_process_stream, fir_calibrate, rs_process_stream, behind the entry point's own null rule (and rs's rate rule).
// One channel's strides are not looked at.  The stride rule's sentence is the entry point's own, whole; so is the tail of
// the overlap sentence.
struct ChannelNouns {
    const char *stride;                 // "channel stride smaller than n"
    const char *elements;               // refuse_misaligned's
    bool in_place;                      // the overlap sentence is refuse_overlap's, "(in-place operation is not supported)" included
};
inline int check_channels(const char *who, const ChannelNouns &nn, size_t n_channels, const void *d_in, size_t n, size_t in_stride, size_t isz,
                          const void *d_out, size_t cap, size_t out_stride, size_t osz, bool tx10)
{
    if (n_channels > 1 && (in_stride < n || out_stride < cap)) {
        set_error("%s: %s", who, nn.stride);
        return SFE_EINVAL;
    }
    size_t in_b = 0, out_b = 0;         // (tx10: out_b counts floats first)
    if (!span_bytes(n_channels - 1, in_stride, n, isz, &in_b) || !span_bytes(n_channels - 1, out_stride, cap, tx10 ? osz / 4 : osz, &out_b))
        return refuse_2_62(who);
    if (tx10) out_b = (out_b / 4 + 1) * 5;
    const Span in{d_in, in_b, isz}, out{d_out, out_b, tx10 ? (size_t)1 : osz};
    int rc = refuse_misaligned(who, nn.elements, {in, out});
    if (rc != SFE_OK) return rc;
    if (tx10 && n_channels > 1 && ((out_stride * (osz / 4)) & 3)) {
        set_error("%s: 10-bit output packs 4 floats per group: out_stride must keep channels on group boundaries", who);
        return SFE_EINVAL;
    }
    if (nn.in_place) return refuse_overlap(who, in, {out});
    if (ranges_overlap(in.p, in.bytes, out.p, out.bytes)) {
        set_error("%s: input and output ranges overlap", who);
        return SFE_EINVAL;
    }
    return SFE_OK;
}

// ==== the byte ranges of the entry points that keep their own sequence of rules, because their shapes fit no family:
// combine (its TX10 and 2^31 rules sit between the shared ones), corr (two peak outputs and an optional metric), mvdr and eig
// (several optional outputs under one compound SFE_ERANGE sentence).  Each is false where a range is not below 2^62: the
// caller then returns refuse_2_62.

// combine: n_streams * M rows of n_in cf32 in; per stream a row of n_out cf32, or of n_out / 2 TX10 groups of 5 bytes, out
inline bool combine_ranges(size_t n_streams, size_t M, bool tx10, const void *d_in, size_t n_in, size_t in_stride, const void *d_out,
                           size_t n_out, size_t out_stride, Span *in, Span *out)
{
    size_t in_b, out_b;
    if (!span_bytes(n_streams * M - 1, in_stride, n_in, 8, &in_b) ||
        !(tx10 ? span_bytes(n_streams - 1, out_stride / 2, n_out / 2, 5, &out_b) : span_bytes(n_streams - 1, out_stride, n_out, 8, &out_b)))
        return false;
    *in = Span{d_in, in_b, 8};
    *out = Span{d_out, out_b, tx10 ? (size_t)1 : (size_t)8};
    return true;
}

// corr: n_streams rows of n_in samples in; n_streams * K rows of `blocks` peak values and indices, and of n_in metric
// values where d_metric is given, out
struct CorrRanges {
    Span in, val, idx, met;
};
inline bool corr_ranges(size_t n_streams, size_t K, size_t isz, const void *d_in, size_t n_in, size_t in_stride, const void *d_val,
                        const void *d_idx, size_t blocks, size_t peak_stride, const void *d_metric, size_t metric_stride, CorrRanges *r)
{
    const size_t rows = n_streams * K;
    size_t in_b, peak_b, met_b = 0;
    if (!span_bytes(n_streams - 1, in_stride, n_in, isz, &in_b) || !span_bytes(rows - 1, peak_stride, blocks, 4, &peak_b) ||
        (d_metric && !span_bytes(rows - 1, metric_stride, n_in, 4, &met_b)))
        return false;
    *r = CorrRanges{Span{d_in, in_b, isz}, Span{d_val, peak_b, 4}, Span{d_idx, peak_b, 4}, Span{d_metric, met_b, 4}};
    return true;
}

// mvdr and eig: M bands of n_rows Gram matrices of `gram` floats in; per row one record of `row` 4-byte words for each output,
// a null one having no bytes.  out[i] is the i-th of outs.
struct RowOut {
    const void *p;
    size_t stride, row;
};
inline bool solver_ranges(size_t M, const void *d_gram, size_t n_rows, size_t in_stride, size_t gram, std::initializer_list<RowOut> outs,
                          Span *in, Span *out)
{
    size_t b;
    if (!span_bytes(M - 1, in_stride, n_rows * gram, 4, &b)) return false;
    *in = Span{d_gram, b, 4};
    for (const RowOut &o : outs) {
        b = 0;
        if (o.p && !span_bytes(n_rows - 1, o.stride, o.row, 4, &b)) return false;
        *out++ = Span{o.p, b, 4};
    }
    return true;
}

}  // namespace sfe
