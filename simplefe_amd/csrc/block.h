// block.h -- what every handle of libsfe_dsp.so is built from: owners of its device memory, pinned host memory (Buf; the
// grow-only GrowScratch and Grown), streams and events, the carried pair (with the history epilogue and load_history of
// the FIR and resample / decimate handles), the device scope of a create, the handle cast,
// the table of the unit circle, the opening of every process_stream and the format setter.  The checks of a call's buffers need no HIP and live in call_checks.h, which
// this includes: the pieces (Span, span_bytes, refuse_*), the one check each of five families of blocks -- rows
// (api_vit.hip, api_reed.hip, api_ldpc.hip, api_crc.hip), windows (api_burst.hip, api_ofdm.hip), frames (api_mod.hip, api_ofdmmod.hip),
// streams (api_chan.hip, api_ddc.hip, api_psd.hip, api_iir.hip, api_polar.hip, api_beam.hip, api_cov.hip), channels
// (api_fir.hip, api_rs.hip) -- and the byte
// ranges of the four that keep their own sequence (api_combine.hip, api_corr.hip, api_mvdr.hip, api_eig.hip).  The FIR, resampler and pipe handles (host.h, api_pipe.hip) and every block's api_*.hip use it.  HOST CODE
// ONLY; host.h includes it.  A handle's struct names its magic as `static constexpr uint32_t MAGIC` and carries `magic` and
// `device`.
#pragma once
#include <math.h>
#include <stdint.h>

#include <initializer_list>
#include <memory>
#include <utility>
#include <vector>

#include "call_checks.h"
#include "common.h"

namespace sfe {

// DeviceGuard: common.h
#define SFE_ON_DEVICE(dev)                                   \
    DeviceGuard guard__(dev);                                \
    if (!guard__.ok) {                                       \
        set_error("cannot select device %d", (int)(dev));    \
        return SFE_EHIP;                                     \
    }

int use_device(int device);                                                    // hipSetDevice with the range / no-GPU checks
bool stream_is_capturing(hipStream_t s);

// ---- memory owned by a handle: freed with it.  DevBuf: device memory; PinnedBuf: pinned host memory
template <class T, bool PINNED>
struct Buf {
    T *p = nullptr;
    Buf() = default;
    Buf(Buf &&o) noexcept : p(std::exchange(o.p, nullptr)) {}
    Buf &operator=(Buf &&o) noexcept       // what this held goes to `o` and is freed with it
    {
        std::swap(p, o.p);
        return *this;
    }
    ~Buf() { release(); }
    void release()
    {
        if (p) (void)(PINNED ? hipHostFree(p) : hipFree(p));
        p = nullptr;
    }
    operator T *() const { return p; }
    int alloc(size_t n)
    {
        SFE_HIP(PINNED ? hipHostMalloc((void **)&p, n * sizeof(T)) : hipMalloc((void **)&p, n * sizeof(T)));
        return SFE_OK;
    }
    int grow(size_t n)      // for a caller that keeps its own capacity: the old buffer goes first (peak memory: one of the two)
    {
        release();
        return alloc(n);
    }
    int upload(const T *src, size_t n)      // (upload, alloc_zero: device buffers only)
    {
        static_assert(!PINNED, "device buffers only");
        SFE_HIP(hipMalloc(&p, n * sizeof(T)));
        SFE_HIP(hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice));
        return SFE_OK;
    }
    int upload(const std::vector<T> &v) { return upload(v.data(), v.size()); }
    int alloc_zero(size_t n)
    {
        static_assert(!PINNED, "device buffers only");
        SFE_HIP(hipMalloc(&p, n * sizeof(T)));
        SFE_HIP(hipMemset(p, 0, n * sizeof(T)));
        return SFE_OK;
    }
};
template <class T> using DevBuf = Buf<T, false>;
template <class T> using PinnedBuf = Buf<T, true>;

// a stream the handle created (a caller's stream is borrowed and stays a raw hipStream_t), an event: destroyed with the handle
struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(const Stream &) = delete;
    Stream &operator=(const Stream &) = delete;
    ~Stream()
    {
        if (s) (void)hipStreamDestroy(s);
    }
    operator hipStream_t() const { return s; }
    int create()
    {
        SFE_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        return SFE_OK;
    }
};
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(const Event &) = delete;
    Event &operator=(const Event &) = delete;
    ~Event()
    {
        if (e) (void)hipEventDestroy(e);
    }
    operator hipEvent_t() const { return e; }
    int create(unsigned flags = hipEventDisableTiming)
    {
        SFE_HIP(hipEventCreateWithFlags(&e, flags));
        return SFE_OK;
    }
};

// Carried state: a call reads cur() and writes next(); the host flips the two after a launch that succeeded.
struct CarriedPair {
    DevBuf<char> b[2];
    size_t bytes = 0;
    int c = 0;
    int alloc_zero(size_t n)
    {
        bytes = n;
        for (auto &d : b) {
            const int rc = d.alloc_zero(n);
            if (rc != SFE_OK) return rc;
        }
        return SFE_OK;
    }
    int zero()
    {
        for (auto &d : b) SFE_HIP(hipMemset(d.p, 0, bytes));
        return SFE_OK;
    }
    template <class T = void> T *cur() const { return reinterpret_cast<T *>(b[c].p); }
    template <class T = void> T *next() const { return reinterpret_cast<T *>(b[c ^ 1].p); }
    void flip() { c ^= 1; }
    // behind a launch that wrote next().  `captured`: a hipGraph names cur(), so the state stays there for good -- the new
    // state is copied back instead of flipping (a replay after an eager call would read the stale buffer)
    int carry(bool captured, hipStream_t s)
    {
        if (captured) SFE_HIP(hipMemcpyAsync(b[c].p, b[c ^ 1].p, bytes, hipMemcpyDeviceToDevice, s));
        else flip();
        return SFE_OK;
    }
};

// ---- the carried history of the FIR and resample / decimate handles: [n_channels][hl] samples of `width` floats
// Behind a call's launches: the state the NEXT call starts from.  `fused`: the main launch already wrote it into
// hist.next().  A captured call (`capturing`) is REPLAYED with the same arguments, so it updates the history IN PLACE,
// behind everything that read the old one -- with n >= hl the carry-over kernel reads `in` only -- and marks the handle:
// a handle one of whose calls sits in a hipGraph keeps its state in hist.cur() for good -- the graph names that buffer --
// so an eager call on such a handle copies the new state back instead of flipping (CarriedPair::carry; a replay after an
// eager call used to read the stale buffer).
inline int carry_history(CarriedPair &hist, bool &captured, const void *d_in, size_t n, size_t in_stride, int hl, int width, int n_channels,
                         int in_u8, bool fused, bool capturing, hipStream_t s)
{
    if (capturing) captured = true;
    if (capturing || !fused) {
        const int rc = launch_history_update(d_in, (long long)n, (long long)in_stride, hist.cur(), capturing ? hist.cur() : hist.next(), hl, width,
                                             n_channels, s, in_u8);
        if (rc != SFE_OK || capturing) return rc;
    }
    return hist.carry(captured, s);
}

// sfe_dsp_fir_load_history / sfe_dsp_rs_load_history over as_handle's result.  Carried state from a halo: the stream is
// about to continue at a sample whose predecessors are d_prev[0 .. n_prev) (float32, the handle's element type, per
// channel at `stride`) -- e.g. the first call of a span when one long stream is cut across GPUs (blkconv.cxx:105-109:
// what the reference carries in m_overlap is determined by exactly these input samples).
template <class H>
int load_history(const char *who, H *p, const void *d_prev, size_t n_prev, size_t stride, hipStream_t s)
{
    if (!p || (n_prev && !d_prev)) {
        set_error("%s: null handle or buffer", who);
        return SFE_EINVAL;
    }
    if (p->n_channels > 1 && stride < n_prev) {
        set_error("%s: channel stride smaller than n_prev", who);
        return SFE_EINVAL;
    }
    int rc = refuse_misaligned(who, "cf32 8 B, f32 4 B", {Span{d_prev, 0, p->data_complex ? (size_t)8 : (size_t)4}});
    if (rc != SFE_OK) return rc;
    SFE_ON_DEVICE(p->device);
    SFE_HIP(hipMemsetAsync(p->hist.cur(), 0, p->hist.bytes, s));        // shorter halos: zeros in front
    if (!n_prev) return SFE_OK;
    rc = launch_history_update(d_prev, (long long)n_prev, (long long)stride, p->hist.cur(), p->hist.next(), p->hl, p->data_complex ? 2 : 1,
                               p->n_channels, s, 0);
    return rc != SFE_OK ? rc : p->hist.carry(p->captured, s);
}

// Scratch of one call that only grows: the one allocation (and device sync) a process_stream may make, when a larger
// call than any before arrives.  Calls already enqueued read the old one: they finish before it is freed.
struct GrowScratch {
    DevBuf<char> d;
    size_t bytes = 0;
    int reserve(size_t need)
    {
        if (need <= bytes) return SFE_OK;
        SFE_HIP(hipDeviceSynchronize());
        bytes = 0;
        const int rc = d.grow(need);
        if (rc == SFE_OK) bytes = need;
        return rc;
    }
    template <class T> T *as() const { return reinterpret_cast<T *>(d.p); }
};

// Memory that only grows, with the capacity it was last given: reserve(n) is a comparison while n fits.  The caller orders
// the regrowth against work in flight (GrowScratch above does so itself) and picks the policy: `to` is the new capacity (exact: n).
// A failed regrowth leaves capacity 0 and nothing to read.  B: a Buf, or several that share one capacity (Mirror; grow(n)).
template <class B>
struct Grown {
    B b;
    size_t cap = 0;
    int reserve(size_t n, size_t to)
    {
        if (n <= cap) return SFE_OK;
        cap = 0;
        const int rc = b.grow(to);
        if (rc == SFE_OK) cap = to;
        return rc;
    }
    int reserve(size_t n) { return reserve(n, n); }
    B *operator->() { return &b; }
};
// a device array and the pinned staging it is uploaded from
template <class T>
struct Mirror {
    DevBuf<T> d;
    PinnedBuf<T> h;
    int grow(size_t n)
    {
        const int rc = d.grow(n);
        return rc != SFE_OK ? rc : h.grow(n);
    }
};

// A create runs on the handle's device and leaves the caller's current device as it found it, on every way out.
struct CreateScope {
    int prev = -1, rc;
    explicit CreateScope(int device)
    {
        (void)hipGetDevice(&prev);
        rc = use_device(device);
    }
    CreateScope(const CreateScope &) = delete;
    CreateScope &operator=(const CreateScope &) = delete;
    ~CreateScope()
    {
        if (rc == SFE_OK && prev >= 0) (void)hipSetDevice(prev);
    }
};

// ---- handles
template <class T>
T *as_handle(void *h, const char *noun)     // nullptr for a null handle (no message) and for a stale or foreign one
{
    T *p = static_cast<T *>(h);
    if (p && p->magic != T::MAGIC) {
        set_error("not a live %s handle", noun);
        return nullptr;
    }
    return p;
}

// the zeroing of sfe_dsp_<block>_reset; the caller clears its own counter when this returns SFE_OK
inline int reset_pairs(int device, std::initializer_list<CarriedPair *> pairs)
{
    SFE_ON_DEVICE(device);
    SFE_HIP(hipDeviceSynchronize());
    for (CarriedPair *q : pairs) {
        const int rc = q->zero();
        if (rc != SFE_OK) return rc;
    }
    SFE_HIP(hipDeviceSynchronize());
    for (CarriedPair *q : pairs) q->c = 0;
    return SFE_OK;
}

// sfe_dsp_<block>_destroy over as_handle's result: a null or foreign handle frees nothing
template <class T>
int destroy_handle(T *p)
{
    if (!p) return SFE_OK;
    DeviceGuard g(p->device);
    (void)hipDeviceSynchronize();
    p->magic = 0;
    delete p;
    return SFE_OK;
}

// ---- exp(sign j 2 pi q / N), q = 0 .. N - 1, N a multiple of 4: rounded once from float64, the quarter turns exact
inline std::vector<v2f> unit_circle(int N, int sign)
{
    std::vector<v2f> tw(N);
    const float s1 = (float)sign, cq[4] = {1.0f, 0.0f, -1.0f, 0.0f}, sq[4] = {0.0f, s1, 0.0f, -s1};
    for (int q = 0; q < N; q++) {
        const double a = 2.0 * M_PI * q / N;
        tw[q] = v2f{(float)cos(a), (float)(sign * sin(a))};
        if (q % (N / 4) == 0) tw[q] = v2f{cq[q / (N / 4)], sq[q / (N / 4)]};
    }
    return tw;
}

// ---- what every process_stream opens with; `who` is the message prefix ("chan_process_stream")
// *n_out is zero whatever follows; nullptr (message set) without a live handle or without n_out
template <class T>
T *stream_handle(T *p, const char *who, size_t *n_out, const char *n_name = "n_out")     // p: as_handle's result
{
    if (n_out) *n_out = 0;
    if (!p || !n_out) {
        set_error("%s: null handle or %s", who, n_name);
        return nullptr;
    }
    return p;
}
// the checks of the buffers that follow: call_checks.h

// sfe_dsp_<block>_set_input_format / _set_output_format where the format is all there is to check: SFE_FMT_F32 clears
// the handle's flag, `other` (SFE_FMT_U8 or SFE_FMT_TX10; `other_name` for the message) sets it.  p: as_handle's result
template <class T>
int set_format(T *p, const char *who, int fmt, int other, const char *other_name, int T::*flag)
{
    if (!p || (fmt != SFE_FMT_F32 && fmt != other)) {
        set_error("%s: null handle or a format other than SFE_FMT_F32 / %s", who, other_name);
        return SFE_EINVAL;
    }
    p->*flag = fmt == other;
    return SFE_OK;
}

// the counter named advances on the host with the carried pair, so a captured call could not be replayed
inline int refuse_capture(const char *who, const char *counter, hipStream_t s)
{
    if (!stream_is_capturing(s)) return SFE_OK;
    set_error("%s: graph capture is not supported (the %s counter lives on the host)", who, counter);
    return SFE_ESTATE;
}

}  // namespace sfe
