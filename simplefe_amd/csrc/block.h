// block.h -- what every handle of libsfe_dsp.so is built from: owners of its device memory, pinned host memory, streams and
// events, the carried pair, the device scope of a create, the handle cast, the table of the unit circle, and the checks
// every process_stream of a streaming block opens with.  The FIR, resampler and pipe handles (host.h, api_pipe.hip) and the
// streaming blocks' (api_chan.hip ... api_mod.hip) all use it.  HOST CODE ONLY; host.h includes it.  A handle's struct names
// its magic as `static constexpr uint32_t MAGIC` and carries `magic` and `device`.
#pragma once
#include <math.h>
#include <stdint.h>

#include <initializer_list>
#include <memory>
#include <utility>
#include <vector>

#include "common.h"

namespace sfe {

// DeviceGuard: common.h
#define SFE_ON_DEVICE(dev)                                   \
    DeviceGuard guard__(dev);                                \
    if (!guard__.ok) {                                       \
        set_error("cannot select device %d", (int)(dev));    \
        return SFE_EHIP;                                     \
    }

bool ranges_overlap(const void *a, size_t an, const void *b, size_t bn);      // [a, a + an) and [b, b + bn) share a byte
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

// the counter named advances on the host with the carried pair, so a captured call could not be replayed
inline int refuse_capture(const char *who, const char *counter, hipStream_t s)
{
    if (!stream_is_capturing(s)) return SFE_OK;
    set_error("%s: graph capture is not supported (the %s counter lives on the host)", who, counter);
    return SFE_ESTATE;
}

}  // namespace sfe
