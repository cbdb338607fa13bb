// test_call_checks.cpp -- csrc/call_checks.h alone, built by a plain host compiler under -fsanitize=address,undefined
// (tests/test_call_checks_host.py): the return code and the whole message of every check, at the boundary values.  The
// header is the only library file included -- it needs no HIP -- and set_error is this program's own.  Pointers are made-up
// integers: nothing is dereferenced.  Every expected message is written out here as the entry point worded it before the
// checks were shared; none is composed from the code under test.  The refusal of a stride that would wrap a byte range
// is asserted here for every entry point that gained it (the streams and channels families; combine, corr, mvdr and eig through the
// functions that compute their ranges): on a GPU a build that forgot it would launch the call.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <utility>

#include "../../simplefe_amd/csrc/call_checks.h"

static char g_msg[512];
namespace sfe {
void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_msg, sizeof g_msg, fmt, ap);
    va_end(ap);
}
}  // namespace sfe
using namespace sfe;

static int g_fails = 0, g_checks = 0;
static void expect(int line, int rc, int code, const char *text)
{
    g_checks++;
    if (rc == code && strcmp(g_msg, text) == 0) return;
    g_fails++;
    printf("line %d: rc %d, message \"%s\"\n         want %d, \"%s\"\n", line, rc, g_msg, code, text);
}
static void expect_true(int line, bool ok)
{
    g_checks++;
    if (ok) return;
    g_fails++;
    printf("line %d: false\n", line);
}
// the message is cleared first: an accepted call must leave it alone ("")
#define CHECK(call, code, text)                 \
    do {                                        \
        g_msg[0] = 0;                           \
        const int rc__ = (call);                \
        expect(__LINE__, rc__, code, text);     \
    } while (0)
#define TRUE(x) expect_true(__LINE__, (x))

static const void *P(uintptr_t a) { return reinterpret_cast<const void *>(a); }
static const size_t T31 = (size_t)1 << 31, T62 = (size_t)1 << 62, T63 = (size_t)1 << 63;

static void test_span_bytes()
{
    size_t b = 77;
    TRUE(!span_bytes(T63, 2, 0, 1, &b) && b == 77);             // rows * stride overflows
    TRUE(!span_bytes(1, SIZE_MAX, 1, 1, &b) && b == 77);        // + tail overflows
    TRUE(!span_bytes(0, 0, T63, 2, &b) && b == 77);             // * elem overflows
    TRUE(span_bytes(0, 0, T62 - 1, 1, &b) && b == T62 - 1);
    TRUE(!span_bytes(0, 0, T62, 1, &b) && b == T62 - 1);
    TRUE(!span_bytes(0, 0, T62 / 2, 2, &b));                    // 2^62 by the last product, no overflow
    TRUE(span_bytes(1, T62 / 2, T62 / 2 - 1, 1, &b) && b == T62 - 1);
    TRUE(span_bytes(2, 100, 7, 8, &b) && b == 207 * 8);
}

static void test_overlap()
{
    TRUE(!ranges_overlap(P(1000), 100, P(1100), 100) && !ranges_overlap(P(1100), 100, P(1000), 100));      // adjacent
    TRUE(ranges_overlap(P(1000), 100, P(1099), 100) && ranges_overlap(P(1099), 100, P(1000), 100));        // one shared byte
    TRUE(!ranges_overlap(P(1000), 100, P(1050), 0) && !ranges_overlap(P(1050), 0, P(1000), 100));          // no bytes, inside
    TRUE(!ranges_overlap(P(0), 0, P(0), 100) && !ranges_overlap(P(1000), 100, nullptr, 0));
    const Span in{P(1000), 100, 1};
    const char *text = "w: input and output ranges overlap (in-place operation is not supported)";
    CHECK(refuse_overlap("w", in, {Span{P(1100), 100, 1}, Span{P(900), 100, 1}}), SFE_OK, "");
    CHECK(refuse_overlap("w", in, {Span{P(1100), 100, 1}, Span{P(1099), 100, 1}}), SFE_EINVAL, text);
    CHECK(refuse_overlap("w", in, {Span{P(901), 100, 1}}), SFE_EINVAL, text);
    CHECK(refuse_overlap("w", in, {Span{P(1050), 0, 4}, Span{nullptr, 0, 4}}), SFE_OK, "");
    CHECK(refuse_overlap("w", Span{P(1050), 0, 1}, {Span{P(1000), 100, 1}}), SFE_OK, "");
    CHECK(refuse_null("w", {P(8), P(16)}), SFE_OK, "");
    CHECK(refuse_null("w", {P(8), nullptr}), SFE_EINVAL, "w: null buffer");
    CHECK(refuse_2_31("w", T31 - 1), SFE_OK, "");
    CHECK(refuse_2_31("w", T31), SFE_EINVAL, "w: n_in = 2147483648 must be below 2^31 per call");
    CHECK(refuse_misaligned("w", "x 8 B", {Span{P(0x1008), 0, 8}, Span{nullptr, 0, 8}, Span{P(0x1001), 0, 1}}), SFE_OK, "");
    CHECK(refuse_misaligned("w", "x 8 B", {Span{P(0x1008), 0, 8}, Span{P(0x1004), 0, 8}}), SFE_EINVAL,
          "w: buffers must be aligned to their element (x 8 B)");
}

static void test_outputs_overlap()
{
    const uintptr_t at[4] = {0x1000, 0x2000, 0x3000, 0x4000};
    auto run = [&](const uintptr_t *a) {
        return refuse_outputs_overlap("w", {Span{P(a[0]), 0x100, 1}, Span{P(a[1]), 0x100, 1}, Span{P(a[2]), 0x100, 1}, Span{P(a[3]), 0x100, 1}});
    };
    CHECK(run(at), SFE_OK, "");
    for (int i = 0; i < 4; i++)
        for (int j = i + 1; j < 4; j++) {
            uintptr_t a[4] = {at[0], at[1], at[2], at[3]};
            a[j] = at[i] + 0xff;            // the last byte of i, and of nothing else
            CHECK(run(a), SFE_EINVAL, "w: the output ranges overlap one another");
            a[j] = at[i] + 0x100;           // adjacent
            CHECK(run(a), SFE_OK, "");
        }
    CHECK(refuse_outputs_overlap("w", {Span{P(0x1000), 0x100, 1}, Span{nullptr, 0, 4}, Span{P(0x1010), 0, 4}}), SFE_OK, "");
    CHECK(refuse_outputs_overlap("w", {}), SFE_OK, "");
}

static void test_check_starts()
{
    const int64_t R = INT64_MAX - ((int64_t)1 << 33) + 1;       // 2^63 - 2^33
    const char *text = "burst: start_base + b * start_step must stay within +-(2^63 - 2^33) for every burst";
    CHECK(check_starts("burst", R, 0, 1), SFE_OK, "");
    CHECK(check_starts("burst", R + 1, 0, 1), SFE_EINVAL, text);
    CHECK(check_starts("burst", -R, 0, 1), SFE_OK, "");
    CHECK(check_starts("burst", -R - 1, 0, 1), SFE_EINVAL, text);
    CHECK(check_starts("burst", INT64_MIN, 0, 1), SFE_EINVAL, text);
    CHECK(check_starts("burst", INT64_MAX, 0, 1), SFE_EINVAL, text);
    CHECK(check_starts("burst", R, INT64_MAX, 1), SFE_OK, "");          // one burst: the step moves nothing
    CHECK(check_starts("burst", 0, R / 2, 3), SFE_OK, "");              // the last burst at R
    CHECK(check_starts("burst", 1, R / 2, 3), SFE_EINVAL, text);        // and one past it
    CHECK(check_starts("burst", 0, -(R / 2), 3), SFE_OK, "");
    CHECK(check_starts("burst", -1, -(R / 2), 3), SFE_EINVAL, text);
    CHECK(check_starts("burst", 0, INT64_MAX, T31 - 1), SFE_EINVAL, text);      // far outside int64: no wrap back into range
    CHECK(check_starts("ofdm", R + 1, 0, 1), SFE_EINVAL, "ofdm: start_base + b * start_step must stay within +-(2^63 - 2^33) for every burst");
}

static void test_check_place()
{
    const int F = 8;
    // the rules in their order
    CHECK(check_place("mod", F, false, false, 1, 0, 0, T31), SFE_EINVAL, "mod: n_out = 2147483648 and n_bursts = 1 must be below 2^31");
    CHECK(check_place("mod", F, false, false, T31, 0, 0, 10), SFE_EINVAL, "mod: n_out = 10 and n_bursts = 2147483648 must be below 2^31");
    CHECK(check_place("mod", F, true, false, T31, 0, 0, 11), SFE_EINVAL, "mod: n_out = 11 and n_bursts = 2147483648 must be below 2^31");
    CHECK(check_place("mod", F, true, false, 1, -1, 0, 11), SFE_EINVAL, "mod: n_out = 11 must be even with SFE_FMT_TX10 (whole 5-byte groups)");
    CHECK(check_place("mod", F, true, false, 0, 0, 0, 11), SFE_EINVAL, "mod: n_out = 11 must be even with SFE_FMT_TX10 (whole 5-byte groups)");
    CHECK(check_place("mod", F, false, false, 0, 0, 0, 11), SFE_OK, "");
    CHECK(check_place("mod", F, true, true, 0, -5, -3, 10), SFE_OK, "");            // no burst: whatever the starts
    CHECK(check_place("mod", F, false, false, 0, INT64_MIN, INT64_MIN, 0), SFE_OK, "");
    CHECK(check_place("mod", F, false, false, 2, -1, 7, 100), SFE_EINVAL, "mod: start_base = -1 must not be negative");
    CHECK(check_place("mod", F, true, true, 2, 1, 7, 100), SFE_EINVAL,
          "mod: start_step = 7 is below the frame's F = 8 samples (frames must not overlap)");
    CHECK(check_place("mod", F, false, false, 2, 0, F - 1, 100), SFE_EINVAL,
          "mod: start_step = 7 is below the frame's F = 8 samples (frames must not overlap)");
    CHECK(check_place("mod", F, false, false, 2, 0, F, 100), SFE_OK, "");
    CHECK(check_place("mod", F, false, false, 1, 0, F - 1, 100), SFE_OK, "");       // one burst: any step
    CHECK(check_place("mod", F, false, false, 1, 92, -1000, 100), SFE_OK, "");
    CHECK(check_place("mod", F, false, false, 1, 92, INT64_MIN, 100), SFE_OK, "");
    CHECK(check_place("mod", F, false, false, 2, 0, F, 16), SFE_OK, "");            // the last frame ends at n_out
    CHECK(check_place("mod", F, false, false, 2, 0, F, 15), SFE_EINVAL, "mod: the last frame ends behind the stream's n_out = 15 samples");
    CHECK(check_place("mod", F, false, false, 1, 92, 0, 100), SFE_OK, "");
    CHECK(check_place("mod", F, false, false, 1, 93, 0, 100), SFE_EINVAL, "mod: the last frame ends behind the stream's n_out = 100 samples");
    CHECK(check_place("mod", F, false, false, 3, 5, INT64_MAX, 100), SFE_EINVAL, "mod: the last frame ends behind the stream's n_out = 100 samples");
    CHECK(check_place("mod", F, false, false, T31 - 1, INT64_MAX, INT64_MAX, T31 - 1), SFE_EINVAL,
          "mod: the last frame ends behind the stream's n_out = 2147483647 samples");
    // whole groups under TX10: ofdmmod's rule, ahead of the frame's end
    CHECK(check_place("ofdmmod", F, true, true, 1, 1, 0, 100), SFE_EINVAL,
          "ofdmmod: start_base = 1 and start_step = 0 must be even with SFE_FMT_TX10 (a frame starts on a 5-byte group)");
    CHECK(check_place("ofdmmod", F, true, true, 2, 0, 9, 100), SFE_EINVAL,
          "ofdmmod: start_base = 0 and start_step = 9 must be even with SFE_FMT_TX10 (a frame starts on a 5-byte group)");
    CHECK(check_place("ofdmmod", F, true, true, 2, 99, 9, 100), SFE_EINVAL,
          "ofdmmod: start_base = 99 and start_step = 9 must be even with SFE_FMT_TX10 (a frame starts on a 5-byte group)");
    CHECK(check_place("ofdmmod", F, true, true, 1, 0, 9, 100), SFE_OK, "");         // one burst: the step is not looked at
    CHECK(check_place("ofdmmod", F, true, true, 2, 2, 10, 100), SFE_OK, "");
    CHECK(check_place("ofdmmod", F, true, false, 1, 1, 0, 100), SFE_OK, "");        // mod: odd starts are its own business
    CHECK(check_place("ofdmmod", F, true, false, 2, 0, 9, 100), SFE_OK, "");
    CHECK(check_place("ofdmmod", F, false, false, 2, 1, 9, 100), SFE_OK, "");
    CHECK(check_place("ofdmmod", F, true, false, 2, 99, 9, 100), SFE_EINVAL, "ofdmmod: the last frame ends behind the stream's n_out = 100 samples");
}

// ---- rows.  The words each block hands over, and what its entry point said before the checks were shared.
static const RowNouns VIT{"n_bursts", "elements of a burst's row", "ceil(n_info / 8) = ", "", "soft values 4 B, symbols 8 B, records and statuses 4 B", 8};
static const RowNouns REED{"n_frames", "bytes read per frame", "the ", " bytes written per frame",
                           "records and statuses 4 B; payloads and frames need none", 8};
static const RowNouns LDPC{"n_words", "elements read per codeword", "the ", " bytes written per codeword",
                           "soft values 4 B, symbols 8 B, records and statuses 4 B; payloads and codewords need none", 12};

struct RowCase {
    const char *who;
    const RowNouns *nn;
    size_t in_row, esz, out_row;
    bool decode;            // status in, record and status out
    const char *count, *null, *short_in, *short_out, *huge, *misaligned, *in_out, *out_out;
};

static void test_rows(const RowCase &c)
{
    const size_t n = 3, in_b = (2 * c.in_row + c.in_row) * c.esz, out_b = 3 * c.out_row, rec_b = n * c.nn->rec_bytes;
    const uintptr_t IN = 0x10000, OUT = 0x20000, SI = 0x30000, REC = 0x40000, ST = 0x50000;
    bool go;
    auto call = [&](size_t n_, uintptr_t in, size_t is, uintptr_t si, uintptr_t out, size_t os, uintptr_t rec, uintptr_t st) {
        go = true;
        if (!c.decode) si = rec = st = 0;
        return check_rows(c.who, *c.nn, n_, P(in), is, c.in_row, c.esz, P(si), P(out), os, c.out_row, P(rec), P(st), &go);
    };
    const size_t is = c.in_row, os = c.out_row;
    CHECK(call(n, IN, is, SI, OUT, os, REC, ST), SFE_OK, "");
    TRUE(go);
    CHECK(call(n, IN, is, 0, OUT, os, 0, 0), SFE_OK, "");           // every optional buffer left out
    TRUE(go);
    CHECK(call(0, 0, 0, 0, 0, 0, 0, 0), SFE_OK, "");
    TRUE(!go);
    CHECK(call(T31, 0, 0, SI, 0, 0, REC, ST), SFE_EINVAL, c.count);
    TRUE(!go);
    CHECK(call(T31 - 1, 0, 0, SI, OUT, 0, REC, ST), SFE_EINVAL, c.null);        // the count passes, the next rule speaks
    CHECK(call(n, 0, is - 1, SI, OUT, os, REC, ST), SFE_EINVAL, c.null);
    CHECK(call(n, IN, is, SI, 0, os - 1, REC, ST), SFE_EINVAL, c.null);
    CHECK(call(n, IN, is - 1, SI, OUT, os, REC, ST), SFE_ERANGE, c.short_in);
    CHECK(call(n, IN, is, SI, OUT, os - 1, REC, ST), SFE_ERANGE, c.short_out);
    CHECK(call(n, IN + 1, T62, SI, OUT, os, REC, ST), SFE_EINVAL, c.huge);
    CHECK(call(n, IN, is, SI, IN, T62, REC, ST), SFE_EINVAL, c.huge);
    CHECK(call(n, IN, SIZE_MAX, SI, OUT, os, REC, ST), SFE_EINVAL, c.huge);
    CHECK(call(1, IN, T62, SI, OUT, T62, REC, ST), SFE_OK, "");     // one row: the strides move nothing
    TRUE(go);
    if (c.esz > 1) {
        CHECK(call(n, IN + c.esz / 2, is, SI, IN, os, REC, ST), SFE_EINVAL, c.misaligned);
        CHECK(call(n, IN + 1, is, SI, OUT, os, REC, ST), SFE_EINVAL, c.misaligned);
    } else {
        CHECK(call(n, IN + 1, is, SI, OUT + 1, os, REC, ST), SFE_OK, "");
    }
    CHECK(call(n, IN, is, SI, OUT + 3, os, REC, ST), SFE_OK, "");   // bytes out: no alignment
    if (c.decode) {
        CHECK(call(n, IN, is, SI + 2, OUT, os, REC, ST), SFE_EINVAL, c.misaligned);
        CHECK(call(n, IN, is, SI, OUT, os, REC + 2, ST), SFE_EINVAL, c.misaligned);
        CHECK(call(n, IN, is, SI, OUT, os, REC, ST + 2), SFE_EINVAL, c.misaligned);
        CHECK(call(n, IN, is, SI, OUT, os, IN, ST + 1), SFE_EINVAL, c.misaligned);
    }
    CHECK(call(n, IN, is, SI, IN + in_b - 1, os, REC, REC), SFE_EINVAL, c.in_out);
    CHECK(call(n, IN, is, SI, IN + in_b, os, REC, ST), SFE_OK, "");
    CHECK(call(n, IN, is, SI, IN - out_b, os, REC, ST), SFE_OK, "");
    CHECK(call(n, IN, is, SI, IN - out_b + 1, os, REC, ST), SFE_EINVAL, c.in_out);
    CHECK(call(n, IN, 2 * is, SI, IN + (5 * is) * c.esz - 1, os, REC, ST), SFE_EINVAL, c.in_out);      // the stride counts
    CHECK(call(n, IN, 2 * is, SI, IN + (5 * is) * c.esz, os, REC, ST), SFE_OK, "");
    if (c.decode) {
        CHECK(call(n, IN, is, SI, OUT, os, IN, ST), SFE_EINVAL, c.in_out);
        CHECK(call(n, IN, is, SI, OUT, os, REC, IN), SFE_EINVAL, c.in_out);
        CHECK(call(n, IN, is, SI, SI + 4 * n - 1, os, REC, ST), SFE_EINVAL, c.in_out);
        CHECK(call(n, IN, is, SI, SI + 4 * n, os, REC, ST), SFE_OK, "");
        CHECK(call(n, IN, is, SI, OUT, os, SI + 8, ST), SFE_EINVAL, c.in_out);
        CHECK(call(n, IN, is, SI, OUT, os, REC, SI), SFE_EINVAL, c.in_out);
        CHECK(call(n, IN, is, SI, OUT, os, OUT, ST), SFE_EINVAL, c.out_out);
        CHECK(call(n, IN, is, SI, OUT, os, REC, OUT), SFE_EINVAL, c.out_out);
        CHECK(call(n, IN, is, SI, OUT, os, REC, REC + rec_b - 4), SFE_EINVAL, c.out_out);         // the record's own width
        CHECK(call(n, IN, is, SI, OUT, os, REC, REC + rec_b), SFE_OK, "");
        CHECK(call(n, IN, is, SI, OUT, os, ST + 4 * n - 4, ST), SFE_EINVAL, c.out_out);
        CHECK(call(n, IN, is, SI, OUT, os, ST + 4 * n, ST), SFE_OK, "");
        CHECK(call(n, IN, is, 0, OUT, os, 0, OUT), SFE_EINVAL, c.out_out);
        CHECK(call(n, IN, is, SI, OUT, 2 * os, REC, (OUT + 5 * os - 1) & ~(uintptr_t)3), SFE_EINVAL, c.out_out);     // the stride counts
        CHECK(call(n, IN, is, SI, OUT, 2 * os, REC, (OUT + 5 * os + 3) & ~(uintptr_t)3), SFE_OK, "");
    }
    TRUE(go);
}

static void test_rows_all()
{
    test_rows(RowCase{"vit_process_stream", &VIT, 40, 4, 5, true, "vit_process_stream: n_bursts = 2147483648 must be below 2^31 per call",
                      "vit_process_stream: null buffer",
                      "vit_process_stream: in_stride 39 < the 40 elements of a burst's row, or out_stride 5 < ceil(n_info / 8) = 5",
                      "vit_process_stream: in_stride 40 < the 40 elements of a burst's row, or out_stride 4 < ceil(n_info / 8) = 5",
                      "vit_process_stream: a stride is so large that its buffer's byte range reaches 2^62",
                      "vit_process_stream: buffers must be aligned to their element (soft values 4 B, symbols 8 B, records and statuses 4 B)",
                      "vit_process_stream: input and output ranges overlap (in-place operation is not supported)",
                      "vit_process_stream: the output ranges overlap one another"});
    test_rows(RowCase{"vit_process_stream", &VIT, 23, 8, 5, true, "vit_process_stream: n_bursts = 2147483648 must be below 2^31 per call",
                      "vit_process_stream: null buffer",
                      "vit_process_stream: in_stride 22 < the 23 elements of a burst's row, or out_stride 5 < ceil(n_info / 8) = 5",
                      "vit_process_stream: in_stride 23 < the 23 elements of a burst's row, or out_stride 4 < ceil(n_info / 8) = 5",
                      "vit_process_stream: a stride is so large that its buffer's byte range reaches 2^62",
                      "vit_process_stream: buffers must be aligned to their element (soft values 4 B, symbols 8 B, records and statuses 4 B)",
                      "vit_process_stream: input and output ranges overlap (in-place operation is not supported)",
                      "vit_process_stream: the output ranges overlap one another"});
    test_rows(RowCase{"reed_encode_stream", &REED, 96, 1, 120, false, "reed_encode_stream: n_frames = 2147483648 must be below 2^31 per call",
                      "reed_encode_stream: null buffer",
                      "reed_encode_stream: in_stride 95 < the 96 bytes read per frame, or out_stride 120 < the 120 bytes written per frame",
                      "reed_encode_stream: in_stride 96 < the 96 bytes read per frame, or out_stride 119 < the 120 bytes written per frame",
                      "reed_encode_stream: a stride is so large that its buffer's byte range reaches 2^62", "",
                      "reed_encode_stream: input and output ranges overlap (in-place operation is not supported)", ""});
    test_rows(RowCase{"reed_process_stream", &REED, 120, 1, 96, true, "reed_process_stream: n_frames = 2147483648 must be below 2^31 per call",
                      "reed_process_stream: null buffer",
                      "reed_process_stream: in_stride 119 < the 120 bytes read per frame, or out_stride 96 < the 96 bytes written per frame",
                      "reed_process_stream: in_stride 120 < the 120 bytes read per frame, or out_stride 95 < the 96 bytes written per frame",
                      "reed_process_stream: a stride is so large that its buffer's byte range reaches 2^62",
                      "reed_process_stream: buffers must be aligned to their element (records and statuses 4 B; payloads and frames need none)",
                      "reed_process_stream: input and output ranges overlap (in-place operation is not supported)",
                      "reed_process_stream: the output ranges overlap one another"});
    test_rows(RowCase{"ldpc_encode_stream", &LDPC, 12, 1, 24, false, "ldpc_encode_stream: n_words = 2147483648 must be below 2^31 per call",
                      "ldpc_encode_stream: null buffer",
                      "ldpc_encode_stream: in_stride 11 < the 12 elements read per codeword, or out_stride 24 < the 24 bytes written per codeword",
                      "ldpc_encode_stream: in_stride 12 < the 12 elements read per codeword, or out_stride 23 < the 24 bytes written per codeword",
                      "ldpc_encode_stream: a stride is so large that its buffer's byte range reaches 2^62", "",
                      "ldpc_encode_stream: input and output ranges overlap (in-place operation is not supported)", ""});
    const char *ldpc_al = "ldpc_process_stream: buffers must be aligned to their element (soft values 4 B, symbols 8 B, records and statuses 4 B; "
                          "payloads and codewords need none)";
    test_rows(RowCase{"ldpc_process_stream", &LDPC, 192, 4, 12, true, "ldpc_process_stream: n_words = 2147483648 must be below 2^31 per call",
                      "ldpc_process_stream: null buffer",
                      "ldpc_process_stream: in_stride 191 < the 192 elements read per codeword, or out_stride 12 < the 12 bytes written per codeword",
                      "ldpc_process_stream: in_stride 192 < the 192 elements read per codeword, or out_stride 11 < the 12 bytes written per codeword",
                      "ldpc_process_stream: a stride is so large that its buffer's byte range reaches 2^62", ldpc_al,
                      "ldpc_process_stream: input and output ranges overlap (in-place operation is not supported)",
                      "ldpc_process_stream: the output ranges overlap one another"});
    test_rows(RowCase{"ldpc_process_stream", &LDPC, 99, 8, 12, true, "ldpc_process_stream: n_words = 2147483648 must be below 2^31 per call",
                      "ldpc_process_stream: null buffer",
                      "ldpc_process_stream: in_stride 98 < the 99 elements read per codeword, or out_stride 12 < the 12 bytes written per codeword",
                      "ldpc_process_stream: in_stride 99 < the 99 elements read per codeword, or out_stride 11 < the 12 bytes written per codeword",
                      "ldpc_process_stream: a stride is so large that its buffer's byte range reaches 2^62", ldpc_al,
                      "ldpc_process_stream: input and output ranges overlap (in-place operation is not supported)",
                      "ldpc_process_stream: the output ranges overlap one another"});
}

// ---- windows
struct WindowCase {
    const char *who, *row_name;
    size_t row, chan_row;       // chan_row 0: the block has no channel output
    const char *n_in, *count, *null, *short_out, *short_status, *short_in, *starts, *huge, *misaligned, *in_out, *out_out;
};

static void test_windows(const WindowCase &c, size_t isz)
{
    const size_t S = 2, n_in = 1000, nb = 3, rows = S * nb, REC = 8;
    const size_t in_b = (n_in + n_in) * isz, ou_b = rows * c.row * 8, ch_b = rows * c.chan_row * 8, re_b = rows * REC * 4, st_b = (nb + nb) * 4;
    struct A {
        size_t S, n_in, in_stride;
        uintptr_t in, idx;
        size_t idx_stride;
        uintptr_t gate;
        size_t gate_stride, nb;
        int64_t base, step;
        uintptr_t out;
        size_t out_stride;
        uintptr_t chan, rec, st;
        size_t st_stride;
    };
    const A good{S, n_in, n_in, 0x100000, 0x200000, nb, 0x300000, nb, nb, 5, 7, 0x400000, c.row, c.chan_row ? (uintptr_t)0x500000 : 0, 0x600000, 0x700000, nb};
    bool go;
    auto call = [&](const A &a) {
        go = true;
        return check_windows(c.who, c.row_name, a.S, isz, P(a.in), a.n_in, a.in_stride, P(a.idx), a.idx_stride, P(a.gate), a.gate_stride, a.nb,
                             a.base, a.step, P(a.out), a.out_stride, c.row, P(a.chan), c.chan_row, P(a.rec), REC, P(a.st), a.st_stride, &go);
    };
    A a = good;
    CHECK(call(a), SFE_OK, "");
    TRUE(go);
    a = good, a.idx = a.gate = a.chan = a.rec = a.st = 0, a.idx_stride = a.gate_stride = a.st_stride = 0;
    CHECK(call(a), SFE_OK, "");         // every optional buffer left out, and its stride with it
    TRUE(go);
    a = good, a.nb = 0, a.in = a.out = 0, a.out_stride = 0;
    CHECK(call(a), SFE_OK, "");
    TRUE(!go);
    a = good, a.n_in = T31, a.nb = T31;
    CHECK(call(a), SFE_EINVAL, c.n_in);
    TRUE(!go);
    a = good, a.nb = T31 / 2, a.in = 0;
    CHECK(call(a), SFE_EINVAL, c.count);
    a = good, a.nb = T31 / 2 - 1, a.n_in = T31 - 1, a.in = 0;
    CHECK(call(a), SFE_EINVAL, c.null);
    a = good, a.in = 0, a.out_stride = c.row - 1;
    CHECK(call(a), SFE_EINVAL, c.null);
    a = good, a.out = 0, a.out_stride = c.row - 1;
    CHECK(call(a), SFE_EINVAL, c.null);
    a = good, a.out_stride = c.row - 1, a.in_stride = n_in - 1;
    CHECK(call(a), SFE_ERANGE, c.short_out);
    a = good, a.st_stride = nb - 1, a.in_stride = n_in - 1;
    CHECK(call(a), SFE_ERANGE, c.short_status);
    a = good, a.st_stride = nb - 1, a.st = 0;
    CHECK(call(a), SFE_OK, "");
    a = good, a.in_stride = n_in - 1, a.base = INT64_MIN;
    CHECK(call(a), SFE_EINVAL, c.short_in);
    a = good, a.S = 1, a.in_stride = 0;
    CHECK(call(a), SFE_OK, "");         // one stream: its stride moves nothing
    a = good, a.base = INT64_MAX - ((int64_t)1 << 33) + 2, a.step = 0, a.in_stride = T62;
    CHECK(call(a), SFE_EINVAL, c.starts);
    a = good, a.base = INT64_MAX - ((int64_t)1 << 33) + 1 - 14, a.in += 1;
    CHECK(call(a), SFE_EINVAL, c.misaligned);           // the last burst at the bound: the starts pass, a later rule speaks
    a.step = 8;
    CHECK(call(a), SFE_EINVAL, c.starts);
    // each stride at 2^62; an absent buffer's stride is not looked at
    a = good, a.in_stride = T62 / isz - n_in + 1, a.in += 1;
    CHECK(call(a), SFE_EINVAL, c.huge);
    a = good, a.idx_stride = T62, a.in += 1;
    CHECK(call(a), SFE_EINVAL, c.huge);
    a.idx = 0, a.in = good.in;
    CHECK(call(a), SFE_OK, "");
    a = good, a.gate_stride = T62;
    CHECK(call(a), SFE_EINVAL, c.huge);
    a.gate = 0;
    CHECK(call(a), SFE_OK, "");
    a = good, a.out_stride = T62;
    CHECK(call(a), SFE_EINVAL, c.huge);
    a = good, a.st_stride = SIZE_MAX;
    CHECK(call(a), SFE_EINVAL, c.huge);
    a.st = 0;
    CHECK(call(a), SFE_OK, "");
    // each buffer off its element's alignment, ahead of any overlap
    a = good, a.in += isz / 2, a.out = a.in;
    CHECK(call(a), SFE_EINVAL, c.misaligned);
    a = good, a.idx += 2, a.out = good.in;
    CHECK(call(a), SFE_EINVAL, c.misaligned);
    a = good, a.gate += 2;
    CHECK(call(a), SFE_EINVAL, c.misaligned);
    a = good, a.out += 4;
    CHECK(call(a), SFE_EINVAL, c.misaligned);
    a = good, a.rec += 2;
    CHECK(call(a), SFE_EINVAL, c.misaligned);
    a = good, a.st += 1;
    CHECK(call(a), SFE_EINVAL, c.misaligned);
    if (c.chan_row) {
        a = good, a.chan += 4;
        CHECK(call(a), SFE_EINVAL, c.misaligned);
    }
    if (isz == 2) {
        a = good, a.in += 2;
        CHECK(call(a), SFE_OK, "");
    }
    // an input against an output, ahead of output against output
    a = good, a.out = good.in + in_b - 8, a.rec = a.st;
    CHECK(call(a), SFE_EINVAL, c.in_out);
    a = good, a.out = good.in + in_b;
    CHECK(call(a), SFE_OK, "");
    a = good, a.out = good.in - ou_b;
    CHECK(call(a), SFE_OK, "");
    a = good, a.out = good.in - ou_b + 8;
    CHECK(call(a), SFE_EINVAL, c.in_out);
    a = good, a.rec = good.idx + (nb + nb) * 4 - 4;
    CHECK(call(a), SFE_EINVAL, c.in_out);
    a = good, a.rec = good.idx + (nb + nb) * 4;
    CHECK(call(a), SFE_OK, "");
    a = good, a.st = good.gate + (nb + nb) * 4 - 4;
    CHECK(call(a), SFE_EINVAL, c.in_out);
    a = good, a.st = good.gate + (nb + nb) * 4;
    CHECK(call(a), SFE_OK, "");
    a = good, a.st = good.in;
    CHECK(call(a), SFE_EINVAL, c.in_out);
    if (c.chan_row) {
        a = good, a.chan = good.in + in_b - 8;
        CHECK(call(a), SFE_EINVAL, c.in_out);
        a = good, a.chan = good.gate - ch_b + 8;
        CHECK(call(a), SFE_EINVAL, c.in_out);
        a = good, a.chan = good.gate - ch_b;
        CHECK(call(a), SFE_OK, "");
    }
    // every pair of outputs; each buffer's extent from its own width
    a = good, a.rec = good.out + ou_b - 4;
    CHECK(call(a), SFE_EINVAL, c.out_out);
    a = good, a.rec = good.out + ou_b;
    CHECK(call(a), SFE_OK, "");
    a = good, a.st = good.out - st_b + 4;
    CHECK(call(a), SFE_EINVAL, c.out_out);
    a = good, a.st = good.out - st_b;
    CHECK(call(a), SFE_OK, "");
    a = good, a.st = good.rec + re_b - 4;
    CHECK(call(a), SFE_EINVAL, c.out_out);
    a = good, a.st = good.rec + re_b;
    CHECK(call(a), SFE_OK, "");
    if (c.chan_row) {
        a = good, a.chan = good.out + ou_b - 8;
        CHECK(call(a), SFE_EINVAL, c.out_out);
        a = good, a.chan = good.out + ou_b;
        CHECK(call(a), SFE_OK, "");
        a = good, a.rec = good.chan + ch_b - 4;
        CHECK(call(a), SFE_EINVAL, c.out_out);
        a = good, a.rec = good.chan + ch_b;
        CHECK(call(a), SFE_OK, "");
        a = good, a.st = good.chan + ch_b - 4;
        CHECK(call(a), SFE_EINVAL, c.out_out);
        a = good, a.chan = good.st - ch_b;
        CHECK(call(a), SFE_OK, "");
    }
    TRUE(go);
}

static void test_windows_all()
{
    const WindowCase burst{"burst_process_stream", "n_sym", 16, 0, "burst_process_stream: n_in = 2147483648 must be below 2^31 per call",
                           "burst_process_stream: n_streams * n_bursts = 2 * 1073741824 must be below 2^31 per call",
                           "burst_process_stream: null buffer",
                           "burst_process_stream: out_stride 15 < n_sym = 16 or status_stride 3 < n_bursts = 3",
                           "burst_process_stream: out_stride 16 < n_sym = 16 or status_stride 2 < n_bursts = 3",
                           "burst_process_stream: in_stride 999 < n_in 1000 with 2 streams",
                           "burst_process_stream: start_base + b * start_step must stay within +-(2^63 - 2^33) for every burst",
                           "burst_process_stream: a stride is so large that its buffer's byte range reaches 2^62",
                           "burst_process_stream: buffers must be aligned to their element (cf32 8 B, u8 (I,Q) pairs 2 B, indices, gates, records and "
                           "statuses 4 B)",
                           "burst_process_stream: input and output ranges overlap (in-place operation is not supported)",
                           "burst_process_stream: the output ranges overlap one another"};
    const WindowCase ofdm{"ofdm_process_stream", "n_data * Nd", 3 * 48, 64, "ofdm_process_stream: n_in = 2147483648 must be below 2^31 per call",
                          "ofdm_process_stream: n_streams * n_bursts = 2 * 1073741824 must be below 2^31 per call",
                          "ofdm_process_stream: null buffer",
                          "ofdm_process_stream: out_stride 143 < n_data * Nd = 144 or status_stride 3 < n_bursts = 3",
                          "ofdm_process_stream: out_stride 144 < n_data * Nd = 144 or status_stride 2 < n_bursts = 3",
                          "ofdm_process_stream: in_stride 999 < n_in 1000 with 2 streams",
                          "ofdm_process_stream: start_base + b * start_step must stay within +-(2^63 - 2^33) for every burst",
                          "ofdm_process_stream: a stride is so large that its buffer's byte range reaches 2^62",
                          "ofdm_process_stream: buffers must be aligned to their element (cf32 8 B, u8 (I,Q) pairs 2 B, indices, gates, records and "
                          "statuses 4 B)",
                          "ofdm_process_stream: input and output ranges overlap (in-place operation is not supported)",
                          "ofdm_process_stream: the output ranges overlap one another"};
    for (size_t isz : {(size_t)8, (size_t)2}) {
        test_windows(burst, isz);
        test_windows(ofdm, isz);
    }
}

// ---- frames
struct FrameCase {
    const char *who;
    FrameNouns nn;
    size_t in_row, ie;
    bool even_starts;       // under TX10
    const char *place, *null, *short_in, *huge, *misaligned, *in_out;
};

static void test_frames(const FrameCase &c, bool tx10)
{
    const int F = 8;
    const size_t nb = 3, n_out = 40, in_b = (2 * c.in_row + c.in_row) * c.ie, out_b = tx10 ? n_out / 2 * 5 : n_out * 8;
    const uintptr_t IN = 0x10000, OUT = 0x20000;
    bool go;
    auto call = [&](uintptr_t in, size_t is, size_t nb_, int64_t base, int64_t step, uintptr_t out, size_t n_out_) {
        go = true;
        return check_frames(c.who, c.nn, F, tx10, tx10 && c.even_starts, P(in), is, c.in_row, c.ie, nb_, base, step, P(out), n_out_, &go);
    };
    const size_t is = c.in_row;
    CHECK(call(IN, is, nb, 0, 16, OUT, n_out), SFE_OK, "");
    TRUE(go);
    CHECK(call(0, 0, 0, -1, -1, 0, 0), SFE_OK, "");             // no stream: nothing to do
    TRUE(!go);
    CHECK(call(0, 0, 0, -1, -1, OUT, n_out), SFE_OK, "");       // no burst: a stream of zeros
    TRUE(go);
    CHECK(call(0, 0, nb, -1, 16, 0, n_out), SFE_EINVAL, c.place);
    TRUE(!go);
    CHECK(call(IN, is - 1, nb, 0, 16, 0, n_out), SFE_EINVAL, c.null);
    CHECK(call(0, is - 1, nb, 0, 16, OUT, n_out), SFE_EINVAL, c.null);
    CHECK(call(IN, is - 1, nb, 0, 16, OUT + 4, n_out), SFE_ERANGE, c.short_in);
    CHECK(call(IN, is - 1, 0, 0, 16, OUT, n_out), SFE_OK, "");          // no burst: the stride is not looked at
    CHECK(call(IN, T62, nb, 0, 16, OUT + 4, n_out), SFE_EINVAL, c.huge);
    CHECK(call(IN, SIZE_MAX, nb, 0, 16, OUT, n_out), SFE_EINVAL, c.huge);
    CHECK(call(IN, T62, 1, 0, 16, OUT, n_out), SFE_OK, "");             // one burst: the stride moves nothing
    if (tx10) {
        CHECK(call(IN, is, nb, 0, 16, OUT + 1, n_out), SFE_OK, "");
    } else {
        CHECK(call(IN, is, nb, 0, 16, OUT + 4, n_out), SFE_EINVAL, c.misaligned);
        CHECK(call(IN, is, nb, 0, 16, IN + 1, n_out), SFE_EINVAL, c.misaligned);
    }
    if (c.ie > 1) {
        CHECK(call(IN + c.ie / 2, is, nb, 0, 16, IN, n_out), SFE_EINVAL, c.misaligned);
        CHECK(call(IN + 4, is, 0, 0, 16, OUT, n_out), SFE_EINVAL, c.misaligned);
    } else {
        CHECK(call(IN + 1, is, nb, 0, 16, OUT, n_out), SFE_OK, "");
    }
    CHECK(call(IN, is, nb, 0, 16, IN, n_out), SFE_EINVAL, c.in_out);
    if (c.ie == 1) {        // to the byte, by the output's own width: 8 bytes a sample, or 5 bytes a pair
        CHECK(call(OUT + out_b, is, nb, 0, 16, OUT, n_out), SFE_OK, "");
        CHECK(call(OUT + out_b - 1, is, nb, 0, 16, OUT, n_out), SFE_EINVAL, c.in_out);
    }
    CHECK(call(OUT + ((out_b + 7) & ~(size_t)7), is, nb, 0, 16, OUT, n_out), SFE_OK, "");
    CHECK(call(OUT + ((out_b - 1) & ~(size_t)7), is, nb, 0, 16, OUT, n_out), SFE_EINVAL, c.in_out);
    CHECK(call(OUT - in_b, is, nb, 0, 16, OUT, n_out), SFE_OK, "");
    CHECK(call(OUT - in_b + 8, is, nb, 0, 16, OUT, n_out), SFE_EINVAL, c.in_out);
    CHECK(call(OUT, is, 0, 0, 16, OUT, n_out), SFE_OK, "");             // no burst: nothing is read
    TRUE(go);
}

static void test_frames_all()
{
    const FrameCase mod{"mod_process_stream",
                        FrameNouns{"ceil(n_info / 8) = ", "", "payloads'", "cf32 output 8 B; TX10 output and payload bytes need none"},
                        5, 1, false, "mod_process_stream: start_base = -1 must not be negative", "mod_process_stream: null buffer",
                        "mod_process_stream: in_stride 4 < ceil(n_info / 8) = 5",
                        "mod_process_stream: in_stride is so large that the payloads' byte range reaches 2^62",
                        "mod_process_stream: buffers must be aligned to their element (cf32 output 8 B; TX10 output and payload bytes need none)",
                        "mod_process_stream: input and output ranges overlap (in-place operation is not supported)"};
    const char *omod_al = "ofdmmod_process_stream: buffers must be aligned to their element (cf32 input and output 8 B; TX10 output and coded bytes "
                          "need none)";
    const FrameCase bits{"ofdmmod_process_stream",
                         FrameNouns{"the ", " bytes a burst reads", "input's", "cf32 input and output 8 B; TX10 output and coded bytes need none"},
                         18, 1, true, "ofdmmod_process_stream: start_base = -1 must not be negative", "ofdmmod_process_stream: null buffer",
                         "ofdmmod_process_stream: in_stride 17 < the 18 bytes a burst reads",
                         "ofdmmod_process_stream: in_stride is so large that the input's byte range reaches 2^62", omod_al,
                         "ofdmmod_process_stream: input and output ranges overlap (in-place operation is not supported)"};
    const FrameCase symbols{"ofdmmod_process_stream",
                            FrameNouns{"the ", " cf32 symbols a burst reads", "input's", "cf32 input and output 8 B; TX10 output and coded bytes need none"},
                            144, 8, true, "ofdmmod_process_stream: start_base = -1 must not be negative", "ofdmmod_process_stream: null buffer",
                            "ofdmmod_process_stream: in_stride 143 < the 144 cf32 symbols a burst reads",
                            "ofdmmod_process_stream: in_stride is so large that the input's byte range reaches 2^62", omod_al,
                            "ofdmmod_process_stream: input and output ranges overlap (in-place operation is not supported)"};
    for (bool tx10 : {false, true}) {
        test_frames(mod, tx10);
        test_frames(bits, tx10);
        test_frames(symbols, tx10);
    }
    // the starts rule reaches the stream call of ofdmmod alone
    bool go;
    CHECK(check_frames("ofdmmod_process_stream", bits.nn, 8, true, true, P(0x10000), 18, 18, 1, 2, 1, 9, P(0x20000), 40, &go), SFE_EINVAL,
          "ofdmmod_process_stream: start_base = 1 and start_step = 9 must be even with SFE_FMT_TX10 (a frame starts on a 5-byte group)");
    CHECK(check_frames("mod_process_stream", mod.nn, 8, true, false, P(0x10000), 5, 5, 1, 2, 1, 9, P(0x20000), 40, &go), SFE_OK, "");
}

// ---- streams.  The words each block hands over, and what its entry point said before the checks were shared.
struct StreamCase {
    const char *who;
    StreamNouns nn;
    size_t n_in, need, in_rows, out_rows, isz, osz;
    const char *n_2_31, *null, *short_out, *short_in, *short_in_one, *wrapped, *misaligned, *in_out;   // short_in_one "": one row's stride is not looked at
};

static void test_streams(const StreamCase &c)
{
    const size_t n = c.n_in, in_b = c.in_rows * n * c.isz, out_b = c.out_rows * c.need * c.osz;
    const uintptr_t IN = 0x100000, OUT = 0x200000;
    bool go;
    auto call = [&](uintptr_t in, size_t n_in, size_t is, size_t in_rows, uintptr_t out, size_t os, size_t need) {
        go = true;
        return check_streams(c.who, c.nn, P(in), n_in, is, in_rows, c.isz, P(out), os, need, c.out_rows, c.osz, &go);
    };
    CHECK(call(IN, n, n, c.in_rows, OUT, c.need, c.need), SFE_OK, "");
    TRUE(go);
    // step 2 ahead of step 3
    CHECK(call(0, 0, 0, c.in_rows, 0, 0, 0), SFE_OK, "");
    TRUE(!go);
    // step 1, ahead of step 3; below the bound the next rule speaks
    if (c.nn.below_2_31) {
        CHECK(call(0, T31, T31, c.in_rows, 0, T31, T31), SFE_EINVAL, c.n_2_31);
        TRUE(!go);
    } else {
        CHECK(call(IN, T31, T31, c.in_rows, IN + (uintptr_t)T31 * 64, T31 / 4, T31 / 4), SFE_OK, "");
        TRUE(go);
    }
    CHECK(call(0, T31 - 1, T31, c.in_rows, OUT, T31, T31), SFE_EINVAL, c.null);
    // step 3 ahead of step 4
    CHECK(call(0, n, n, c.in_rows, OUT, c.need - 1, c.need), SFE_EINVAL, c.null);
    CHECK(call(IN, n, n, c.in_rows, 0, c.need - 1, c.need), SFE_EINVAL, c.null);
    TRUE(!go);
    // step 4 ahead of step 5
    CHECK(call(IN, n, n - 1, c.in_rows, OUT, c.need - 1, c.need), SFE_ERANGE, c.short_out);
    TRUE(!go);
    // step 5 ahead of step 6
    CHECK(call(IN, n, n - 1, c.in_rows, OUT, T62, c.need), SFE_EINVAL, c.short_in);
    if (c.short_in_one[0]) {
        CHECK(call(IN, n, 0, 1, OUT, c.need, c.need), SFE_EINVAL, c.short_in_one);
    } else {
        CHECK(call(IN, n, 0, 1, OUT, c.need, c.need), SFE_OK, "");
        CHECK(call(IN, n, T62, 1, OUT, c.need, c.need), SFE_OK, "");                 // one row: the stride moves nothing
        TRUE(go);
    }
    // step 6 ahead of step 7: the input's range, then the output's, at 2^62 bytes and at the last element below
    CHECK(call(IN + 1, n, T62 / c.isz - n, 2, OUT, c.need, c.need), SFE_EINVAL, c.wrapped);
    TRUE(!go);
    CHECK(call(IN, n, T62 / c.isz - n - 1, 2, IN - out_b, c.need, c.need), SFE_OK, "");
    TRUE(go);
    CHECK(call(IN, n, T62, 2, OUT, c.need, c.need), SFE_EINVAL, c.wrapped);         // * elem overflows
    CHECK(call(IN, n, SIZE_MAX, 2, OUT, c.need, c.need), SFE_EINVAL, c.wrapped);    // + tail overflows
    if (c.in_rows > 2) CHECK(call(IN, n, T63, c.in_rows, OUT, c.need, c.need), SFE_EINVAL, c.wrapped);      // rows * stride overflows
    if (c.out_rows > 1) {
        CHECK(call(IN + 1, n, n, c.in_rows, OUT, T62 / c.osz / (c.out_rows - 1), c.need), SFE_EINVAL, c.wrapped);
        CHECK(call(IN, n, n, c.in_rows, OUT, SIZE_MAX, c.need), SFE_EINVAL, c.wrapped);
        if (c.out_rows > 2) CHECK(call(IN, n, n, c.in_rows, OUT, T63, c.need), SFE_EINVAL, c.wrapped);
    } else {
        CHECK(call(IN, n, n, c.in_rows, OUT, T62, c.need), SFE_OK, "");
    }
    // step 7 ahead of step 8
    CHECK(call(IN + c.isz / 2, n, n, c.in_rows, IN, c.need, c.need), SFE_EINVAL, c.misaligned);
    CHECK(call(IN, n, n, c.in_rows, OUT + c.osz / 2, c.need, c.need), SFE_EINVAL, c.misaligned);
    if (c.isz == 2) CHECK(call(IN + 2, n, n, c.in_rows, OUT, c.need, c.need), SFE_OK, "");
    // step 8, to the element, and the strides count
    CHECK(call(IN, n, n, c.in_rows, IN + in_b - c.osz, c.need, c.need), SFE_EINVAL, c.in_out);
    TRUE(!go);
    CHECK(call(IN, n, n, c.in_rows, IN + in_b, c.need, c.need), SFE_OK, "");
    CHECK(call(IN, n, n, c.in_rows, IN - out_b, c.need, c.need), SFE_OK, "");
    CHECK(call(IN, n, n, c.in_rows, IN - out_b + c.osz, c.need, c.need), SFE_EINVAL, c.in_out);
    CHECK(call(IN, n, 2 * n, c.in_rows, IN + in_b, c.need, c.need), SFE_EINVAL, c.in_out);
    CHECK(call(IN, n, 2 * n, c.in_rows, IN + (2 * c.in_rows - 1) * n * c.isz, c.need, c.need), SFE_OK, "");
    CHECK(call(IN, n, n, c.in_rows, IN - (2 * c.out_rows - 1) * c.need * c.osz + c.osz, 2 * c.need, c.need), SFE_EINVAL, c.in_out);
    CHECK(call(IN, n, n, c.in_rows, IN - (2 * c.out_rows - 1) * c.need * c.osz, 2 * c.need, c.need), SFE_OK, "");
    TRUE(go);
}

static const char CF_U8[] = "cf32 8 B, u8 (I,Q) pairs 2 B", CF_U8_F[] = "cf32 8 B, u8 (I,Q) pairs 2 B, float32 4 B";
static const char CF_U8_ROWS[] = "cf32 8 B, u8 (I,Q) pairs 2 B, float32 rows 4 B", DDC_EL[] = "cf32 8 B, real float 4 B, u8 (I,Q) pairs 2 B";

static void test_streams_all()
{
    // chan: M 4, D 4, two streams; the only block without the 2^31 rule
    const StreamCase chan{"chan_process_stream", StreamNouns{"n_out ", CF_U8, false, true}, 64, 16, 2, 8, 8, 8, "", "chan_process_stream: null buffer",
                          "chan_process_stream: out_stride 15 < n_out 16", "chan_process_stream: in_stride 63 < n_in 64 with 2 streams", "",
                          "chan_process_stream: the strides take a byte range to 2^62",
                          "chan_process_stream: buffers must be aligned to their element (cf32 8 B, u8 (I,Q) pairs 2 B)",
                          "chan_process_stream: input and output ranges overlap (in-place operation is not supported)"};
    // ddc: D 3, K 2, two streams
    const StreamCase ddc{"ddc_process_stream", StreamNouns{"n_out ", DDC_EL, true, true}, 192, 64, 2, 4, 8, 8,
                         "ddc_process_stream: n_in = 2147483648 must be below 2^31 per call", "ddc_process_stream: null buffer",
                         "ddc_process_stream: out_stride 63 < n_out 64", "ddc_process_stream: in_stride 191 < n_in 192 with 2 streams", "",
                         "ddc_process_stream: the strides take a byte range to 2^62",
                         "ddc_process_stream: buffers must be aligned to their element (cf32 8 B, real float 4 B, u8 (I,Q) pairs 2 B)",
                         "ddc_process_stream: input and output ranges overlap (in-place operation is not supported)"};
    // psd: N 256, hop 128, n_avg 2, eight segments: four rows
    const StreamCase psd{"psd_process_stream", StreamNouns{"n_rows * n_fft = ", CF_U8_ROWS, true, true}, 1024, 1024, 2, 2, 8, 4,
                         "psd_process_stream: n_in = 2147483648 must be below 2^31 per call", "psd_process_stream: null buffer",
                         "psd_process_stream: out_stride 1023 < n_rows * n_fft = 1024", "psd_process_stream: in_stride 1023 < n_in 1024 with 2 streams", "",
                         "psd_process_stream: the strides take a byte range to 2^62",
                         "psd_process_stream: buffers must be aligned to their element (cf32 8 B, u8 (I,Q) pairs 2 B, float32 rows 4 B)",
                         "psd_process_stream: input and output ranges overlap (in-place operation is not supported)"};
    const StreamCase iir{"iir_process_stream", StreamNouns{"n_in = ", CF_U8_F, true, true}, 64, 64, 2, 2, 8, 8,
                         "iir_process_stream: n_in = 2147483648 must be below 2^31 per call", "iir_process_stream: null buffer",
                         "iir_process_stream: out_stride 63 < n_in = 64", "iir_process_stream: in_stride 63 < n_in 64 with 2 streams", "",
                         "iir_process_stream: the strides take a byte range to 2^62",
                         "iir_process_stream: buffers must be aligned to their element (cf32 8 B, u8 (I,Q) pairs 2 B, float32 4 B)",
                         "iir_process_stream: input and output ranges overlap (in-place operation is not supported)"};
    const StreamCase polar{"polar_process_stream", StreamNouns{"n_in = ", CF_U8_F, true, true}, 64, 64, 2, 2, 8, 4,
                           "polar_process_stream: n_in = 2147483648 must be below 2^31 per call", "polar_process_stream: null buffer",
                           "polar_process_stream: out_stride 63 < n_in = 64", "polar_process_stream: in_stride 63 < n_in 64 with 2 streams", "",
                           "polar_process_stream: the strides take a byte range to 2^62",
                           "polar_process_stream: buffers must be aligned to their element (cf32 8 B, u8 (I,Q) pairs 2 B, float32 4 B)",
                           "polar_process_stream: input and output ranges overlap (in-place operation is not supported)"};
    // beam: S 2, B 3, M 2
    const StreamCase beam{"beam_process_stream", StreamNouns{"n_in = ", CF_U8, true, false}, 64, 64, 4, 6, 8, 8,
                          "beam_process_stream: n_in = 2147483648 must be below 2^31 per call", "beam_process_stream: null buffer",
                          "beam_process_stream: out_stride 63 < n_in = 64", "beam_process_stream: in_stride 63 < n_in 64",
                          "beam_process_stream: in_stride 0 < n_in 64", "beam_process_stream: the strides take a byte range to 2^62",
                          "beam_process_stream: buffers must be aligned to their element (cf32 8 B, u8 (I,Q) pairs 2 B)",
                          "beam_process_stream: input and output ranges overlap (in-place operation is not supported)"};
    // cov: S 2, M 1, two rows of (2 S)^2 floats
    const StreamCase cov{"cov_process_stream", StreamNouns{"n_rows * (2 n_in_streams)^2 = ", CF_U8_ROWS, true, false}, 64, 32, 2, 1, 8, 4,
                         "cov_process_stream: n_in = 2147483648 must be below 2^31 per call", "cov_process_stream: null buffer",
                         "cov_process_stream: out_stride 31 < n_rows * (2 n_in_streams)^2 = 32", "cov_process_stream: in_stride 63 < n_in 64",
                         "cov_process_stream: in_stride 0 < n_in 64", "cov_process_stream: the strides take a byte range to 2^62",
                         "cov_process_stream: buffers must be aligned to their element (cf32 8 B, u8 (I,Q) pairs 2 B, float32 rows 4 B)",
                         "cov_process_stream: input and output ranges overlap (in-place operation is not supported)"};
    for (const StreamCase *c : {&chan, &ddc, &psd, &iir, &polar, &beam, &cov}) {
        test_streams(*c);
        StreamCase u8 = *c;
        u8.isz = 2;
        test_streams(u8);
    }
    StreamCase real = ddc;          // the real inputs of ddc and iir, and iir's real output
    real.isz = 4;
    test_streams(real);
    real = iir, real.isz = real.osz = 4;
    test_streams(real);
    // one byte below 2^62, with a byte for an element
    bool go = false;
    CHECK(check_streams(chan.who, chan.nn, P(0x100000), 64, T62 - 65, 2, 1, P(0x80000), 16, 16, 8, 8, &go), SFE_OK, "");
    TRUE(go);
    CHECK(check_streams(chan.who, chan.nn, P(0x100000), 64, T62 - 64, 2, 1, P(0x80000), 16, 16, 8, 8, &go), SFE_EINVAL, chan.wrapped);
    TRUE(!go);
    // psd and cov: a call that completes no row writes nothing, so an output inside the input overlaps nothing
    for (const StreamCase *c : {&psd, &cov}) {
        go = false;
        CHECK(check_streams(c->who, c->nn, P(0x100000), c->n_in, c->n_in, c->in_rows, 8, P(0x100010), 0, 0, c->out_rows, 4, &go), SFE_OK, "");
        TRUE(go);
        CHECK(check_streams(c->who, c->nn, P(0x100000), c->n_in, c->n_in, c->in_rows, 8, P(0x100010), 4, 4, c->out_rows, 4, &go), SFE_EINVAL, c->in_out);
        CHECK(check_streams(c->who, c->nn, P(0x100000), c->n_in, c->n_in, c->in_rows, 8, P(0x100012), 0, 0, c->out_rows, 4, &go), SFE_EINVAL,
              c->misaligned);           // its alignment is still looked at
    }
}

// ---- channels: the FIR handle's two entry points and the resampler's, behind their own null rules.  The sentences are the
// entry points' as they read before the family was shared; the 2^62 rule is the one they gained.
static const ChannelNouns FIR_NOUNS{"channel stride smaller than n", "cf32 8 B, f32 4 B, u8 (I,Q) pairs 2 B; 10-bit output: none", true};
static const ChannelNouns RS_NOUNS{"channel stride smaller than the channel (in_stride >= n_in, out_stride >= out_cap)",
                                   "cf32 8 B, f32 4 B, u8 (I,Q) pairs 2 B", false};
struct ChannelCase {
    const char *who;
    const ChannelNouns *nn;
    size_t n, cap, isz, osz;
    const char *stride, *wrapped, *misaligned, *in_out;
};

static void test_channels(const ChannelCase &c)
{
    const size_t n = c.n, cap = c.cap, C3 = 3, in_b = C3 * n * c.isz, out_b = C3 * cap * c.osz;
    const uintptr_t IN = 0x100000, OUT = 0x200000;
    auto call = [&](size_t ch, uintptr_t in, size_t n_, size_t is, uintptr_t out, size_t cap_, size_t os) {
        return check_channels(c.who, *c.nn, ch, P(in), n_, is, c.isz, P(out), cap_, os, c.osz, false);
    };
    CHECK(call(C3, IN, n, n, OUT, cap, cap), SFE_OK, "");
    // the stride rule, for several channels only, ahead of the 2^62 rule
    CHECK(call(C3, IN, n, n - 1, OUT, cap, T62), SFE_EINVAL, c.stride);
    CHECK(call(C3, IN, n, T62, OUT, cap, cap - 1), SFE_EINVAL, c.stride);
    CHECK(call(1, IN, n, 0, OUT, cap, 0), SFE_OK, "");
    CHECK(call(1, IN, n, T62, OUT, cap, SIZE_MAX), SFE_OK, "");             // one channel: the strides move nothing
    // the 2^62 rule, ahead of the alignment rule: each range at 2^62 bytes and at the last element below; the three ways to wrap
    CHECK(call(2, IN + 1, n, T62 / c.isz - n, OUT, cap, cap), SFE_EINVAL, c.wrapped);
    CHECK(call(2, IN, n, T62 / c.isz - n - 1, IN - 2 * cap * c.osz, cap, cap), SFE_OK, "");
    CHECK(call(2, IN, n, T62, OUT, cap, cap), SFE_EINVAL, c.wrapped);                   // * elem overflows (or reaches 2^62)
    CHECK(call(2, IN, n, SIZE_MAX, OUT, cap, cap), SFE_EINVAL, c.wrapped);              // + tail overflows
    CHECK(call(C3, IN, n, T63, OUT, cap, cap), SFE_EINVAL, c.wrapped);                  // rows * stride overflows
    CHECK(call(2, IN + 1, n, n, OUT, cap, T62 / c.osz - cap), SFE_EINVAL, c.wrapped);
    CHECK(call(2, IN - 2 * n * c.isz, n, n, IN, cap, T62 / c.osz - cap - 1), SFE_OK, "");
    CHECK(call(2, IN, n, n, OUT, cap, T62), SFE_EINVAL, c.wrapped);
    CHECK(call(2, IN, n, n, OUT, cap, SIZE_MAX), SFE_EINVAL, c.wrapped);
    CHECK(call(C3, IN, n, n, OUT, cap, T63), SFE_EINVAL, c.wrapped);
    CHECK(call(1, IN, T62 / c.isz, 0, OUT, cap, 0), SFE_EINVAL, c.wrapped);             // one channel: the samples themselves
    CHECK(call(1, IN, n, 0, OUT, T62 / c.osz, 0), SFE_EINVAL, c.wrapped);
    CHECK(call(1, IN, T62 / c.isz - 1, 0, IN - 8 * cap, cap, 0), SFE_OK, "");
    // the alignment rule ahead of the overlap rule
    if (c.isz > 1) CHECK(call(C3, IN + c.isz / 2, n, n, IN, cap, cap), SFE_EINVAL, c.misaligned);
    else CHECK(call(C3, IN + 1, n, n, OUT, cap, cap), SFE_OK, "");
    CHECK(call(C3, IN, n, n, IN + c.osz / 2, cap, cap), SFE_EINVAL, c.misaligned);
    if (c.isz == 2) CHECK(call(C3, IN + 2, n, n, OUT, cap, cap), SFE_OK, "");
    // the overlap rule, to the element, and the strides count
    CHECK(call(C3, IN, n, n, IN + ((in_b - 1) & ~(c.osz - 1)), cap, cap), SFE_EINVAL, c.in_out);
    CHECK(call(C3, IN, n, n, IN + ((in_b + c.osz - 1) & ~(c.osz - 1)), cap, cap), SFE_OK, "");
    CHECK(call(C3, IN, n, n, IN - out_b, cap, cap), SFE_OK, "");
    CHECK(call(C3, IN, n, n, IN - out_b + c.osz, cap, cap), SFE_EINVAL, c.in_out);
    CHECK(call(C3, IN, n, 2 * n, IN + 8 * ((5 * n * c.isz - 1) / 8), cap, cap), SFE_EINVAL, c.in_out);
    CHECK(call(C3, IN, n, 2 * n, IN + 8 * ((5 * n * c.isz + 7) / 8), cap, cap), SFE_OK, "");
    CHECK(call(C3, IN, n, n, IN - (4 * cap + cap) * c.osz + c.osz, cap, 2 * cap), SFE_EINVAL, c.in_out);
    CHECK(call(C3, IN, n, n, IN - (4 * cap + cap) * c.osz, cap, 2 * cap), SFE_OK, "");
}

// the FIR's 10-bit output: 4 floats in 5 bytes, one group more than the floats fill; `width` floats per sample
static void test_channels_tx10(const char *who, size_t isz, size_t width, const char *groups, const char *wrapped, const char *misaligned,
                               const char *in_out)
{
    const size_t n = 1000, osz = 4 * width;
    const uintptr_t IN = 0x100000, OUT = 0x200000;
    auto call = [&](size_t ch, uintptr_t in, size_t is, uintptr_t out, size_t os) {
        return check_channels(who, FIR_NOUNS, ch, P(in), n, is, isz, P(out), n, os, osz, true);
    };
    CHECK(call(3, IN, n, OUT + 1, n), SFE_OK, "");                      // bytes out: no alignment
    if (isz > 1) CHECK(call(3, IN + isz / 2, n, OUT, n + 1), SFE_EINVAL, misaligned);       // ahead of the group rule
    // channels on group boundaries: out_stride * width a multiple of 4, ahead of the overlap rule; one channel: any stride
    CHECK(call(3, IN, n, IN, n + 1), SFE_EINVAL, groups);
    if (width == 1) CHECK(call(3, IN, n, OUT, n + 2), SFE_EINVAL, groups);
    else CHECK(call(3, IN, n, OUT, n + 2), SFE_OK, "");
    CHECK(call(3, IN, n, OUT, n + 4), SFE_OK, "");
    CHECK(call(1, IN, n, OUT, n + 1), SFE_OK, "");
    // the range: ((channels - 1) * out_stride + n) * width floats, a group of 5 bytes for every 4 and one more
    for (size_t ch : {(size_t)1, (size_t)3}) {
        const size_t os = n + 24, bytes = (((ch - 1) * os + n) * width / 4 + 1) * 5;
        if (isz == 1) {
            CHECK(call(ch, OUT + bytes, n, OUT, os), SFE_OK, "");
            CHECK(call(ch, OUT + bytes - 1, n, OUT, os), SFE_EINVAL, in_out);
        }
        CHECK(call(ch, OUT + ((bytes + 7) & ~(size_t)7), n, OUT, os), SFE_OK, "");
        CHECK(call(ch, OUT + ((bytes - 1) & ~(size_t)7), n, OUT, os), SFE_EINVAL, in_out);
        CHECK(call(ch, IN, n, IN + ch * n * isz, os), SFE_OK, "");
        CHECK(call(ch, IN, n, IN + ch * n * isz - 1, os), SFE_EINVAL, in_out);
    }
    // the floats of the range reach 2^62
    CHECK(call(2, IN, n, OUT, T62 / width - n), SFE_EINVAL, wrapped);
    CHECK(call(2, OUT + 0x10000, n, OUT, T62 / width - n - 4), SFE_EINVAL, in_out);      // below it: a range that long lies over all that follows
    CHECK(call(3, IN, n, OUT, T63), SFE_EINVAL, wrapped);
}

static void test_channels_all()
{
    for (const char *who : {"fir_process_stream", "fir_calibrate"}) {
        char stride[128], wrapped[128], misaligned[192], in_out[160], groups[192];
        snprintf(stride, sizeof stride, "%s: channel stride smaller than n", who);
        snprintf(wrapped, sizeof wrapped, "%s: the strides take a byte range to 2^62", who);
        snprintf(misaligned, sizeof misaligned, "%s: buffers must be aligned to their element (cf32 8 B, f32 4 B, u8 (I,Q) pairs 2 B; 10-bit output: none)",
                 who);
        snprintf(in_out, sizeof in_out, "%s: input and output ranges overlap (in-place operation is not supported)", who);
        snprintf(groups, sizeof groups, "%s: 10-bit output packs 4 floats per group: out_stride must keep channels on group boundaries", who);
        // cf32 -> cf32, f32 -> cf32 (complex taps), f32 -> f32, u8 pairs -> cf32, u8 -> f32
        for (auto sz : {std::pair<size_t, size_t>{8, 8}, {4, 8}, {4, 4}, {2, 8}, {1, 4}})
            test_channels(ChannelCase{who, &FIR_NOUNS, 1024, 1024, sz.first, sz.second, stride, wrapped, misaligned, in_out});
        for (auto sz : {std::pair<size_t, size_t>{8, 2}, {4, 1}, {2, 2}, {1, 1}}) test_channels_tx10(who, sz.first, sz.second, groups, wrapped, misaligned, in_out);
    }
    // the resampler: out_cap outputs per channel may be written; its own, shorter overlap sentence
    for (auto sz : {std::pair<size_t, size_t>{8, 8}, {4, 4}, {2, 8}, {1, 4}})
        for (size_t cap : {(size_t)1024, (size_t)520, (size_t)3000})
            test_channels(ChannelCase{"rs_process_stream", &RS_NOUNS, 1024, cap, sz.first, sz.second,
                                      "rs_process_stream: channel stride smaller than the channel (in_stride >= n_in, out_stride >= out_cap)",
                                      "rs_process_stream: the strides take a byte range to 2^62",
                                      "rs_process_stream: buffers must be aligned to their element (cf32 8 B, f32 4 B, u8 (I,Q) pairs 2 B)",
                                      "rs_process_stream: input and output ranges overlap"});
}

// ---- the four entry points that keep their own sequence: their byte ranges, at ordinary and at wrapping strides
static void test_own_ranges()
{
    CHECK(refuse_2_62("mvdr_process_stream"), SFE_EINVAL, "mvdr_process_stream: the strides take a byte range to 2^62");
    CHECK(refuse_2_62("occ_process_stream"), SFE_EINVAL, "occ_process_stream: the strides take a byte range to 2^62");
    const void *I = P(0x100000), *O = P(0x200000);
    Span in{}, out{};
    // combine: n_streams * M rows of n_in cf32 in; a row of n_out cf32, or of n_out / 2 groups of 5 bytes, per stream out
    TRUE(combine_ranges(2, 4, false, I, 64, 100, O, 256, 300, &in, &out));
    TRUE(in.p == I && in.bytes == (7 * 100 + 64) * 8 && in.align == 8 && out.p == O && out.bytes == (300 + 256) * 8 && out.align == 8);
    TRUE(combine_ranges(2, 4, true, I, 64, 100, O, 256, 300, &in, &out));
    TRUE(in.bytes == (7 * 100 + 64) * 8 && out.bytes == (150 + 128) * 5 && out.align == 1);
    TRUE(combine_ranges(1, 4, false, I, 64, 64, O, 256, T62, &in, &out) && out.bytes == 256 * 8);     // one stream: its stride moves nothing
    TRUE(!combine_ranges(1, 2, false, I, 64, T62 / 2, O, 256, 300, &in, &out));         // (2^61 + n) * 8 would come out as 8 n
    TRUE(!combine_ranges(2, 4, false, I, 64, T62 / 8, O, 256, 300, &in, &out));
    TRUE(!combine_ranges(2, 4, false, I, 64, T62, O, 256, 300, &in, &out));             // rows * stride
    TRUE(!combine_ranges(1, 4, false, I, 64, SIZE_MAX / 3, O, 256, 300, &in, &out));    // + tail
    TRUE(!combine_ranges(2, 4, false, I, 64, 100, O, 256, T62 / 8, &in, &out));
    TRUE(!combine_ranges(2, 4, true, I, 64, 100, O, 256, T62, &in, &out));
    TRUE(combine_ranges(2, 4, false, I, 64, 100, O, 256, T62 / 8 - 257, &in, &out) && out.bytes == T62 - 8);
    // corr: n_streams rows in; n_streams * K rows of peaks, twice, and of the optional metric
    CorrRanges c;
    TRUE(corr_ranges(2, 3, 8, I, 1000, 1100, O, P(0x300000), 4, 5, P(0x400000), 1200, &c));
    TRUE(c.in.bytes == 2100 * 8 && c.in.align == 8 && c.val.bytes == (5 * 5 + 4) * 4 && c.idx.bytes == c.val.bytes && c.val.p == O &&
         c.idx.p == P(0x300000) && c.met.bytes == (5 * 1200 + 1000) * 4 && c.met.align == 4);
    TRUE(corr_ranges(2, 3, 2, I, 1000, 1100, O, P(0x300000), 4, 5, nullptr, T62, &c) && c.in.bytes == 2100 * 2 && c.met.bytes == 0);   // no metric: its stride is not looked at
    TRUE(!corr_ranges(2, 3, 8, I, 1000, T62 / 8, O, P(0x300000), 4, 5, P(0x400000), 1200, &c));
    TRUE(!corr_ranges(2, 3, 2, I, 1000, T62, O, P(0x300000), 4, 5, P(0x400000), 1200, &c));
    TRUE(!corr_ranges(2, 3, 8, I, 1000, 1100, O, P(0x300000), 4, T62 / 4, P(0x400000), 1200, &c));
    TRUE(!corr_ranges(2, 3, 8, I, 1000, 1100, O, P(0x300000), 4, T62, P(0x400000), 1200, &c));
    TRUE(!corr_ranges(2, 3, 8, I, 1000, 1100, O, P(0x300000), 4, 5, P(0x400000), T62 / 4, &c));
    TRUE(!corr_ranges(2, 3, 8, I, 1000, 1100, O, P(0x300000), 4, 5, P(0x400000), SIZE_MAX / 5, &c));
    TRUE(corr_ranges(1, 1, 8, I, 1000, T62, O, P(0x300000), 4, T62, P(0x400000), T62, &c) && c.in.bytes == 8000);      // one row each
    // mvdr and eig: M bands of n_rows grams in; per row one record of each output, the optional ones null
    Span o[4];
    TRUE(solver_ranges(3, I, 5, 100, 16, {RowOut{O, 50, 40}, RowOut{nullptr, T62, 7}, RowOut{P(0x300000), 9, 3}}, &in, o));
    TRUE(in.bytes == (2 * 100 + 5 * 16) * 4 && in.align == 4 && o[0].p == O && o[0].bytes == (4 * 50 + 40) * 4 && o[1].p == nullptr &&
         o[1].bytes == 0 && o[2].bytes == (4 * 9 + 3) * 4 && o[2].align == 4);
    TRUE(!solver_ranges(3, I, 5, T62 / 4, 16, {RowOut{O, 50, 40}}, &in, o));
    TRUE(!solver_ranges(3, I, 5, T62, 16, {RowOut{O, 50, 40}}, &in, o));
    TRUE(!solver_ranges(3, I, 5, 100, 16, {RowOut{O, T62 / 4, 40}}, &in, o));
    TRUE(!solver_ranges(3, I, 5, 100, 16, {RowOut{O, 50, 40}, RowOut{P(0x300000), T62 / 16, 7}}, &in, o));
    TRUE(!solver_ranges(3, I, 5, 100, 16, {RowOut{O, 50, 40}, RowOut{P(0x300000), 9, 3}, RowOut{P(0x400000), 9, 3}, RowOut{P(0x500000), T63, 3}}, &in, o));
    TRUE(solver_ranges(1, I, 1, T62, 16, {RowOut{O, T62, 40}}, &in, o) && in.bytes == 64 && o[0].bytes == 160);       // one band, one row
}

int main()
{
    test_span_bytes();
    test_overlap();
    test_outputs_overlap();
    test_check_starts();
    test_check_place();
    test_rows_all();
    test_windows_all();
    test_frames_all();
    test_streams_all();
    test_channels_all();
    test_own_ranges();
    if (g_fails) {
        printf("call checks: %d of %d FAILED\n", g_fails, g_checks);
        return 1;
    }
    printf("call checks ok: %d checks\n", g_checks);
    return 0;
}
