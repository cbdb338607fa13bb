/*
 * sfe_dsp.h -- C ABI of libsfe_dsp.so, the MI355X (gfx950) implementation of simpleFE's
 * libdsp sample-stream hot path: blkconv (FIR block convolution), resample and decimate
 * (polyphase interpolating resamplers).
 *
 * This is the drop-in boundary.  The reference has no FFI/plugin registry; what it exposes
 * for this path is the C++ class surface of its static library `Libdsp`
 * (libdsp/CMakeLists.txt:16-21; classes at libdsp/blkconv.h:35-62, libdsp/resample.h:33-61,
 * libdsp/decimate.h:33-63) and its SWIG projection (libdsp/test/pydsp.i:16-22).  Every entry
 * point below names the reference member it stands behind; include/blkconv.h, resample.h,
 * decimate.h are header-only classes with the reference's names and signatures that forward
 * here, so existing callers (examples/bpsk/bpsk.cxx:125-164, libdsp/test/test_blkconv.cxx)
 * compile unchanged.  INTEGRATION.md shows the binding a maintainer would add.
 *
 * Conventions
 *   - plain C types only: pointers, sizes, ints.  No HIP, torch or C++ types.
 *   - every function returns an int status: 0 (SFE_OK) or a negative SFE_E* code;
 *     sfe_dsp_last_error() gives the message of the calling thread's last failure.
 *   - one handle == one stream of samples with its own filter state, exactly like one
 *     reference object.  Handles are not thread-safe; callers serialise per handle, the rule
 *     the reference has (examples/bpsk/bpsk.cxx:132-170).
 *   - sfe_stream_t is a hipStream_t passed as void* (NULL = the default stream).  The
 *     *_stream entry points are asynchronous on that stream; the host-pointer entry points
 *     (class-compatible) return when the result is in host memory.
 *   - complex samples are interleaved (re, im) float32 pairs -- gr_complex, as gr-simplefe
 *     uses (gr-simplefe/lib/source_c_impl.cc:46,123-128).  libdsp itself is real-only
 *     (libdsp/blkconv.h:38-48); complex data is the composition SURVEY.md 8(a) row A0 defines.
 *   - there is NO CPU fallback: without a usable GPU the create calls fail with SFE_ENODEV.
 */
#ifndef SFE_DSP_H_
#define SFE_DSP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SFE_OK       0
#define SFE_EINVAL  (-1)  /* bad argument */
#define SFE_ENOMEM  (-2)  /* host or device allocation failed */
#define SFE_EHIP    (-3)  /* a HIP runtime call failed (message has the HIP error string) */
#define SFE_ENODEV  (-4)  /* no usable gfx950 device */
#define SFE_ESTATE  (-5)  /* call not valid in the handle's current state */
#define SFE_ERANGE  (-6)  /* output buffer too small */

typedef void *sfe_stream_t;   /* hipStream_t */
typedef void *sfe_fir_t;      /* opaque: one FIR stream (blkconv) */
typedef void *sfe_pipe_t;     /* opaque: pipelined host streaming over one FIR handle */
typedef void *sfe_rs_t;       /* opaque: one resample/decimate stream */
typedef void *sfe_timer_t;    /* opaque: a pair of HIP events */

/* ------------------------------------------------------------------ runtime / plumbing */
const char *sfe_dsp_version(void);
const char *sfe_dsp_last_error(void);
int sfe_dsp_device_count(int *count);
/* The calling thread's current device (HIP's notion: hipSetDevice / hipGetDevice).  Handles name
 * their device at create and switch to it on every call, so these two matter only to what has no
 * device argument: sfe_dsp_malloc and friends, and the drop-in classes blkconv / resample /
 * decimate (the class headers under include/), whose reference constructors have no such argument -- an object lives on
 * the device that is current when it is constructed (0 unless the caller chose another).
 * get_device: SFE_ENODEV without a GPU. */
int sfe_dsp_set_device(int device);
int sfe_dsp_get_device(int *device);
int sfe_dsp_sync(sfe_stream_t stream);                       /* hipStreamSynchronize */
int sfe_dsp_malloc(void **dptr, size_t bytes);               /* device memory */
int sfe_dsp_free(void *dptr);
int sfe_dsp_host_alloc(void **hptr, size_t bytes);           /* pinned host memory */
int sfe_dsp_host_free(void *hptr);
int sfe_dsp_memcpy_h2d(void *dptr, const void *hptr, size_t bytes, sfe_stream_t stream);
int sfe_dsp_memcpy_d2h(void *hptr, const void *dptr, size_t bytes, sfe_stream_t stream);
int sfe_dsp_memset(void *dptr, int value, size_t bytes, sfe_stream_t stream);
/* HIP-event timer on `stream` (bench.py's roofline leg): start/stop record events there */
int sfe_dsp_timer_create(sfe_timer_t *t);
int sfe_dsp_timer_start(sfe_timer_t t, sfe_stream_t stream);
int sfe_dsp_timer_stop(sfe_timer_t t, sfe_stream_t stream);
int sfe_dsp_timer_elapsed_ms(sfe_timer_t t, float *ms);      /* synchronises on stop */
int sfe_dsp_timer_destroy(sfe_timer_t t);
/* Synthetic stream generator: float i of the run is
 * (int32(hash32(seed, channel, first + i)) >> 8) * 2^-23; simplefe_amd/synth.py is the
 * host twin. */
int sfe_dsp_synth_fill(void *dptr, uint64_t n_floats, uint32_t seed, uint32_t channel,
                       uint64_t first, sfe_stream_t stream);

/* ------------------------------------------------------------------------ FIR (blkconv)
 * y[n] = sum_{k < n_taps} h[k] x[n-k], zero initial state, state carried across calls:
 * the net effect of blkconv::process() over a stream (libdsp/blkconv.cxx:77-110), for
 * real or complex data and real or complex taps. */
#define SFE_FIR_ALGO_AUTO    0
#define SFE_FIR_ALGO_DIRECT  1   /* time-domain, LDS-staged (short filters; evidence kernel) */
#define SFE_FIR_ALGO_FFT     2   /* in-LDS 4096-point FFT overlap-save (the headline kernel) */

/* Replaces blkconv::blkconv(float *taps, int n_taps, int fft_len)   libdsp/blkconv.cxx:34-75.
 *   taps          n_taps floats, or n_taps (re,im) pairs when taps_complex; copied.
 *   data_complex  0: real float32 samples (libdsp's own case); 1: interleaved cf32.
 *   n_channels    independent streams sharing the taps, each with its own state (>= 1).
 *   block_hint    the caller's fft_len: only fixes the size of the class-compatible host
 *                 block, blk = block_hint + 1 - n_taps (blkconv.cxx:47); 0 = no host block.
 *   device        HIP device ordinal. */
int sfe_dsp_fir_create(const float *taps, int n_taps, int taps_complex, int data_complex,
                       int n_channels, int block_hint, int device, sfe_fir_t *out);

/* The same with a tap vector PER CHANNEL (what 64 reference objects with 64 different filters are):
 *   taps  [n_channels][n_taps] floats ([n_channels][n_taps] (re,im) pairs when taps_complex); copied.
 * Complex float32 streams, the FFT path (any n_taps it takes); one launch covers all channels: a
 * workgroup holds its channel's spectrum in registers as for a shared filter and reloads it when
 * the next transform it draws belongs to another channel (+3 % at 64 x 2^24).  No host block. */
int sfe_dsp_fir_create_per_channel(const float *taps, int n_taps, int taps_complex, int n_channels,
                                   int device, sfe_fir_t *out);
/* Host-only (no GPU): how a tap count is served by the 4096-point kernel -- the overlap of one
 * transform (a multiple of 256), the number of tap partitions (one launch each; 1 for any filter
 * a single transform overlaps economically, i.e. up to ~2800 taps) and the samples a transform
 * advances.  The reference's analogue is the caller's choice of fft_len (blkconv.cxx:47-48:
 * blk = fft_len + 1 - n_taps); here it is chosen by cost.  SFE_ERANGE beyond 1024 partitions. */
int sfe_dsp_fir_plan(int n_taps, int *overlap, int *partitions, int *advance);
/* Replaces get_process_buf()/get_blksize()  libdsp/blkconv.h:40-47: a pinned host buffer
 * owned by the handle, stable for its lifetime; the caller writes and reads [0, blk). */
int sfe_dsp_fir_host_buffer(sfe_fir_t h, float **buf, int *blk);
/* Replaces blkconv::process()  libdsp/blkconv.cxx:77-110: filters the blk samples in the
 * host buffer in place (H2D, kernel, D2H, synchronous); overlap state is carried. */
int sfe_dsp_fir_process_block(sfe_fir_t h);
/* Bulk device-resident form of the same law (the measured path): n samples per channel,
 * channel c at d_in + c*in_stride and d_out + c*out_stride (strides in samples; pass n for
 * packed; with n_channels > 1 both must be >= n).  The input and output byte ranges must not
 * overlap at all (SFE_EINVAL).  Asynchronous on `stream`.  Output is complex when data or taps
 * are complex, else real.  Buffers are aligned to their element: 8 bytes for complex float32,
 * 4 for real float32; with SFE_FMT_U8 input d_in needs 2-byte alignment for (I,Q) pairs and
 * none for real streams (16-byte aligned streams take the faster wide-lane request); with
 * SFE_FMT_TX10 output d_out needs none. */
int sfe_dsp_fir_process_stream(sfe_fir_t h, const void *d_in, void *d_out, size_t n,
                               size_t in_stride, size_t out_stride, sfe_stream_t stream);
/* Host-pointer form of the bulk law for ONE channel and any n: H2D, kernel, D2H through pinned
 * staging owned by the handle, synchronous, state carried.  This is what a GNU Radio
 * work(noutput_items, in, out) adapter calls (include/gr_sfe/): gr-simplefe's blocks hand
 * host buffers of scheduler-chosen length (gr-simplefe/lib/source_c_impl.cc:134-153). */
int sfe_dsp_fir_process_host(sfe_fir_t h, const void *in, void *out, size_t n);
/* One stream cut into spans: before a span's first call, hand the handle the
 * samples that precede the span -- d_prev[0 .. n_prev), float32 in the handle's element type, per
 * channel at `stride` samples; n_prev >= n_taps-1 reproduces the uncut stream exactly, fewer are
 * taken as preceded by zeros.  This is the reference's whole carried state: m_overlap is a
 * function of exactly those n_taps-1 inputs (libdsp/blkconv.cxx:105-109).  With cuts on multiples
 * of the transform advance (3840 for <= 257 taps) and n_prev >= the transform overlap (n_taps-1
 * rounded up to a multiple of 256) the spans' outputs are bit-identical to the one-handle
 * result; otherwise equal to float32 rounding.  Asynchronous on `stream`. */
int sfe_dsp_fir_load_history(sfe_fir_t h, const void *d_prev, size_t n_prev, size_t stride,
                             sfe_stream_t stream);
int sfe_dsp_fir_set_algo(sfe_fir_t h, int algo);
/* How the rows of an aligned complex float32 stream reach the FFT kernel's transform: guarded
 * register loads, LDS-DMA requested early, or LDS-DMA into a wave-private exchange layout
 * (DESIGN.md 4.1).  Same arithmetic, bit-identical output; which is fastest differs by a few
 * percent between devices of one pool and from run to run.  A stream call NEVER measures (round
 * 4; round 3's first large call blocked for ~100 ms to do so): it runs what set_variant fixed,
 * else what an earlier sfe_dsp_fir_calibrate chose for its (device, channels, size class,
 * overlap, per-channel taps), else register loads.
 * sfe_dsp_fir_calibrate is the measurement, made when the caller asks: it times every variant
 * over the caller's own buffers -- a call shaped like the stream calls to come: same n, strides
 * and channel count; d_out receives the filtered d_in each time -- in interleaved rounds for at
 * least 80 ms of launches, the last nine counted, SYNCHRONOUSLY on `stream`, and the process
 * remembers the choice for that shape: register loads unless another variant's median is more
 * than 1 % ahead.  It does not advance the stream: carried state and position are as before.
 * `chosen` (may be NULL) receives the variant.  Refused inside a hipGraph capture (SFE_ESTATE).
 * get_variant: what the handle's last bulk call ran, how many measurements this handle made, and
 * (ms_by_variant: 3 floats, may be NULL) the medians of its last measurement.
 * forget_calibrations drops the process-wide memory.  No reference counterpart: blkconv has one
 * code path (libdsp/blkconv.cxx:77-110). */
#define SFE_FIR_VARIANT_AUTO          (-1)
#define SFE_FIR_VARIANT_REGISTER_LOADS  0
#define SFE_FIR_VARIANT_LDS_DMA         1
#define SFE_FIR_VARIANT_WAVE_PRIVATE    2
int sfe_dsp_fir_set_variant(sfe_fir_t h, int variant);
int sfe_dsp_fir_get_variant(sfe_fir_t h, int *last_variant, int *calibrations, float *ms_by_variant);
int sfe_dsp_fir_forget_calibrations(void);
int sfe_dsp_fir_calibrate(sfe_fir_t h, const void *d_in, void *d_out, size_t n, size_t in_stride,
                          size_t out_stride, sfe_stream_t stream, int *chosen);
/* Host calls (blkconv::process() on the object's buffer, sfe_dsp_fir_process_host) of at most
 * max_samples samples let the kernel read and write pinned host memory itself -- one stream
 * operation instead of copy-in, launch, copy-out (default 2^20 samples; 0 = always the DMA copies).
 * Has no reference counterpart (the reference's buffer, libdsp/blkconv.h:44-47, is plain host
 * memory); a tuning knob of the compatibility path.  Set before the first process_host call. */
int sfe_dsp_fir_set_zero_copy_max(sfe_fir_t h, size_t max_samples);
/* Pipelined host streaming for scheduler-sized calls.  A GNU Radio scheduler
 * hands a block a few thousand items per work() call (gr-simplefe/lib/sink_c_impl.cc:157-174,
 * source_c_impl.cc:134-153); one synchronous round trip per call is launch/sync bound.  A pipe
 * over a single-channel FIR handle (float32 items, or u8 wire-format items in when the handle's
 * input format is SFE_FMT_U8; float32 items out, or -- output format SFE_FMT_TX10 -- the 10-bit
 * transmit wire format: an output ITEM is then one 5-byte group = 2 complex / 4 real samples, only
 * whole groups are ever sent on their way) collects pushed items in pinned batches of
 * `batch_items` (0 = 262144) and keeps up to four batches in flight on three streams (copy in,
 * filter, copy out); pull hands out finished items in order.  Item k out is the filter's output
 * for item k in: no delay is inserted, only latency.  While a pipe exists, drive its handle only
 * through the pipe: the pipe sized its batches from the handle's item formats, so the handle's
 * format setters that would change them, and its destroy call, return SFE_ESTATE until the pipe
 * is destroyed.
 *   push  copies up to n_items in; *n_taken < n_items means every batch is in flight: pull first.
 *   pull  copies up to max_items finished items out.  wait = 0: only what has already arrived;
 *         1: block for the oldest batch in flight; 2: also send a partly filled batch on its way
 *         and block for it (end of stream / drain).
 *   pending  items pushed and not yet pulled. */
int sfe_dsp_fir_pipe_create(sfe_fir_t fir, size_t batch_items, sfe_pipe_t *out);
/* The same pipe over a single-channel float32 resample / decimate handle at a fixed `rate`
 * ({resample,decimate}::process called chunk after chunk, resample.cxx:85-153): push takes input
 * items, pull hands out the outputs of finished batches -- as many as the reference object would
 * have produced for those inputs.  batch_items is rounded up to whole `blksize`-sample reference
 * calls, so the result is the bulk call's (sfe_dsp_rs_process_stream, incl. sfe_dsp_rs_set_exact)
 * for any rate.  A partly filled batch sent on its way early (pull with wait = 2) is cut on a whole
 * number of blksize-sample calls when the step rate*upsample is not integer-valued -- where a
 * reference caller's call would end -- and what is left (less than one call) stays for the next
 * batch unless it is all there is (then it goes out as the short last call a reference caller
 * makes at the end of a stream).  For an integer-valued step the items do not depend on the cuts.
 * Declared after sfe_rs_t below. */
int sfe_dsp_pipe_push(sfe_pipe_t p, const void *in, size_t n_items, size_t *n_taken);
int sfe_dsp_pipe_pull(sfe_pipe_t p, void *out, size_t max_items, int wait, size_t *n_got);
int sfe_dsp_pipe_pending(sfe_pipe_t p, size_t *items);
/* The same pipe without the two host copies -- what get_process_buf() is to blkconv (libdsp/blkconv.h:44-47:
 * the caller works in the object's own buffer): the producer writes its items straight into the pipe's pinned
 * input batch and the consumer reads finished items in place in the pinned output batch (a callback that
 * receives device samples, simpleFE.c:625-653, or a generator such as bpsk.cxx:145-159 has no buffer of its own
 * to copy from).  May be mixed freely with push / pull on the same pipe; same items, same order.
 *   acquire  *buf = where the next item goes, *room_items = how many fit before the batch is sent on its way
 *            (0, *buf NULL: every batch is in flight -- take finished items out first).  The pointer is valid until
 *            the next commit / push on this pipe, or a pull / peek with wait = 2 (which may send the open batch on
 *            its way and move what is left of it).
 *   commit   n_items (<= room) have been written at the acquired pointer; a full batch is sent on its way.
 *   peek     *out = the oldest finished items, *n_items of them contiguous (0: none ready); wait as for pull.
 *            The pointer is valid until they are released.
 *   release  n_items (<= what peek reported) have been consumed. */
int sfe_dsp_pipe_acquire(sfe_pipe_t p, void **buf, size_t *room_items);
int sfe_dsp_pipe_commit(sfe_pipe_t p, size_t n_items);
int sfe_dsp_pipe_peek(sfe_pipe_t p, const void **out, size_t *n_items, int wait);
int sfe_dsp_pipe_release(sfe_pipe_t p, size_t n_items);
int sfe_dsp_pipe_destroy(sfe_pipe_t p);
/* Fused receive converter: with SFE_FMT_U8 the bulk call reads the device
 * wire format directly -- u8 offset binary, one byte per real sample or an (I,Q) byte pair per
 * complex sample -- converting (b-128)*(1/127) on load exactly as fill_rx_buffer does
 * (gr-simplefe/lib/source_c_impl.cc:121-132, source_f_impl.cc:120-129): 2 bytes instead of 8
 * per complex sample from HBM and no separate conversion pass.  in_stride stays in samples.
 * Applies to *_process_stream only. */
#define SFE_FMT_F32 0
#define SFE_FMT_U8  1
int sfe_dsp_fir_set_input_format(sfe_fir_t h, int fmt);
/* Fused transmit converter: with SFE_FMT_TX10 the bulk call writes the device's transmit wire
 * format instead of floats -- ((short)(x*511)+512)&0x3FF, 4 floats packed in 5 bytes exactly as
 * fill_tx_buffer / convert_samples_to_bytes do on the host (gr-simplefe/lib/sink_f_impl.cc:117-143,
 * sink_c_impl.cc:118-144, examples/bpsk/bpsk.cxx:76-101).  Real stream (real taps): 4 samples per
 * group, d_out receives (n/4)*5 bytes per channel, channel c at byte offset c*(out_stride/4)*5.
 * Complex stream: a group is 2 samples (re, im, re, im), d_out receives (n/2)*5 bytes per
 * channel, channel c at byte offset c*(out_stride/2)*5.  Only whole groups are emitted, as the
 * reference does.  The stream leaves the GPU at 1.25 (real) / 2.5 (complex) instead of 4 / 8
 * bytes per sample. */
#define SFE_FMT_TX10 2
int sfe_dsp_fir_set_output_format(sfe_fir_t h, int fmt);
/* Zero the carried state (a fresh blkconv object: blkconv.cxx:52-55). */
int sfe_dsp_fir_reset(sfe_fir_t h);
/* Replaces blkconv::~blkconv()  libdsp/blkconv.cxx:113-122. */
int sfe_dsp_fir_destroy(sfe_fir_t h);

/* ------------------------------------------------- channel groups: one process, several GPUs
 * The reference's multi-channel form is one object per stream (libdsp/blkconv.h:35-62): channels
 * are independent, so they shard across devices with no exchange.  A group makes
 * that partition inside the library for a caller that owns several GPUs in ONE process:
 *   channels are cut into n_devices contiguous blocks -- block k holds channels
 *   [k*base + min(k, extra), ...) with base = n_channels / n_devices, extra = n_channels %
 *   n_devices, the first `extra` blocks one channel longer -- block k lives on devices[k] (a
 *   device may be named more than once) as an ordinary handle with a stream of its own there.
 * create: taps as sfe_dsp_fir_create's, or (per_channel != 0) [n_channels][n_taps] as
 *   sfe_dsp_fir_create_per_channel's (then the data are complex).  n_devices <= n_channels.
 * process_stream: d_in[k] / d_out[k] are block k's buffers ON devices[k], channel-major with the
 *   given strides, n samples per channel.  The launches go to every device before anything waits
 *   (asynchronous on the blocks' own streams); sync waits for all of them.  A call that fails after
 *   some blocks have taken their launch leaves the blocks out of step: further calls return
 *   SFE_ESTATE until _reset (a failure at the first block -- bad arguments -- has moved nothing).
 * shard: what block k is -- its device, first channel, channel count, the underlying handle (for
 *   sfe_dsp_fir_set_variant / load_history / calibrate ... on it) and its stream (to order the
 *   caller's copies with the block's launches).  Any out pointer may be NULL.
 * The result equals ONE handle over all n_channels on one device, bit for bit. */
typedef void *sfe_fir_group_t;
int sfe_dsp_fir_group_create(const float *taps, int n_taps, int taps_complex, int data_complex, int per_channel,
                             int n_channels, const int *devices, int n_devices, sfe_fir_group_t *out);
int sfe_dsp_fir_group_shards(sfe_fir_group_t g, int *n_shards);
int sfe_dsp_fir_group_shard(sfe_fir_group_t g, int shard, int *device, int *first_channel, int *n_channels,
                            sfe_fir_t *handle, sfe_stream_t *stream);
int sfe_dsp_fir_group_process_stream(sfe_fir_group_t g, const void *const *d_in, void *const *d_out, size_t n,
                                     size_t in_stride, size_t out_stride);
int sfe_dsp_fir_group_sync(sfe_fir_group_t g);
int sfe_dsp_fir_group_reset(sfe_fir_group_t g);
int sfe_dsp_fir_group_destroy(sfe_fir_group_t g);

/* -------------------------------------------------------------- resample / decimate
 * Polyphase interpolating resampler: outputs at upsampled-grid instants t (float32
 * recurrence t += rate*upsample), pos = floor(t), mu = t - pos,
 *   out = s(pos)*(1-mu) + mu*s(pos+1),  s(p) = sum_j taps[p%U + j*U] * x[p/U - j]
 * (libdsp/resample.cxx:85-153, libdsp/decimate.cxx:69-140; the two classes give identical
 * output, libdsp/test/test_decimate.py:36). */
#define SFE_RS_RESAMPLE 0   /* accepts rate >= 1/upsample  (resample.cxx:91) */
#define SFE_RS_DECIMATE 1   /* accepts rate >= 1           (decimate.cxx:75) */

/* Replaces resample::resample / decimate::decimate (float *taps, int n_taps, int upsample,
 * int blksize)   libdsp/resample.cxx:37-69, libdsp/decimate.cxx:37-59. */
int sfe_dsp_rs_create(const float *taps, int n_taps, int upsample, int blksize,
                      int data_complex, int n_channels, int device, int mode, sfe_rs_t *out);
/* Replaces {resample,decimate}::process(float *in, int n_in, float *out, int out_len,
 * float rate)   libdsp/resample.cxx:85-153, libdsp/decimate.cxx:69-129.  Host pointers,
 * one channel, synchronous.  Same parameter checks, same messages on stdout and *n_out = 0
 * (resample.cxx:91-98, decimate.cxx:75-87); same leftover / time-recurrence state. */
int sfe_dsp_rs_process(sfe_rs_t h, const float *in, int n_in, float *out, int out_len,
                       float rate, int *n_out);
/* Bulk device-resident form: consumes n_in samples per channel, writes *n_out samples per
 * channel (same count for every channel), equal to what the reference object produces when
 * fed the same stream in chunks of `blksize`.  When fl(rate*upsample) is integer-valued the
 * result does not depend on the chunking and one closed-form launch is used; otherwise the
 * float32 time recurrence is replayed on the host, chunk by chunk, and uploaded.
 * Fails with SFE_ERANGE if out_cap is too small (nothing is written).  Asynchronous.
 * Strides are in samples; with n_channels > 1, in_stride >= n_in and out_stride >= out_cap
 * (up to out_cap outputs per channel may be written).  Buffers are aligned to their element
 * (complex float32 8 bytes, real float32 4, SFE_FMT_U8 (I,Q) pairs 2, real u8 none) and the
 * input and output byte ranges -- (n_channels-1)*stride + n_in resp. out_cap elements -- must
 * not overlap; violations return SFE_EINVAL before anything is launched.  Any such alignment gives the same bits; channels whose
 * first sample sits on a 16-byte boundary (sfe_dsp_malloc memory, strides that are multiples of 16 bytes) take the kernels that fetch
 * their tiles by 16-byte DMA lanes -- 15-35 % faster at ratios without a compile-time kernel, up to 3x for u8 input.
 * SFE_FMT_U8 input is accepted at every rate the float32 path takes: where no kernel converts on load (steps of more than 64 samples, more
 * than 8 outputs per period, a general rate with a small blksize) the call converts its bytes once into a scratch buffer the handle owns and
 * grows (4 x the call's input bytes; not while the stream is being captured) and runs the float32 path -- the same bits. */
int sfe_dsp_rs_process_stream(sfe_rs_t h, const void *d_in, size_t n_in, size_t in_stride,
                              void *d_out, size_t out_cap, size_t out_stride, float rate,
                              size_t *n_out, sfe_stream_t stream);
/* Which kernel the bulk path (fused numerics) takes.  Integer-valued steps -- AUTO: the calibrated
 * rule of DESIGN.md 4.2c (transform-domain kernel for long filters on long calls, else a tiled direct
 * kernel: a compile-time (inputs, outputs)-per-period instantiation or, for any other ratio up to
 * 64 : 8, the runtime-shape one).  DIRECT: never a transform-domain kernel.  FFT: the
 * transform-domain kernel wherever the shape is instantiated.  MFMA: the f32 matrix-pipe form of the
 * direct kernel (measured slower, kept as evidence: DESIGN.md 4.2b).
 * Any other step (the general rate) -- AUTO: float32 calls (complex or real) of >= 65536 samples
 * with >= 12 taps per phase take the 4096-point transform kernel (all phases of every
 * input sample by one forward and `upsample` inverse transforms, blended by the reference's own
 * (pos, mu) sequence; a real stream's transforms carry two blocks each), at any rate the class
 * accepts -- below 1 too, down to 1 / upsample; FFT: at any size; DIRECT and the exact mode: the
 * direct kernel.  u8 streams (SFE_FMT_U8) at such a step ALWAYS take the transform kernel, which
 * converts on load (the direct kernels have no u8 form: the exact mode and DIRECT return
 * SFE_ESTATE for them).  The number of outputs per call is the reference's in every case.
 * The library reads no environment variable. */
#define SFE_RS_ALGO_AUTO    0
#define SFE_RS_ALGO_DIRECT  1
#define SFE_RS_ALGO_FFT     2
#define SFE_RS_ALGO_MFMA    3
int sfe_dsp_rs_set_algo(sfe_rs_t h, int algo);
/* exact = 1: separate multiply and add in the reference's order (bit-exact with the CPU
 * classes); exact = 0 (default for *_stream): fused multiply-add, same order. */
int sfe_dsp_rs_set_exact(sfe_rs_t h, int exact);
/* As sfe_dsp_fir_set_input_format, for the integer-step bulk path (fused numerics). */
int sfe_dsp_rs_set_input_format(sfe_rs_t h, int fmt);
/* One stream cut into spans.  load_history: as sfe_dsp_fir_load_history (the resamplers'
 * m_history, resample.h:49-59 / decimate.h:50-59; phase_len samples suffice).  seek: put the time
 * state {pos, mu, leftover} (resample.h:55-59) where a reference object stands after consuming
 * `first_sample` samples from a fresh start -- closed form, available only when fl(rate*upsample) is
 * integer-valued (both BASELINE resampler configs); otherwise SFE_ESTATE: the float32 recurrence
 * t += rate*U (resample.cxx:129-150) must be carried, which get_state / set_state do (a span's
 * final state is the next span's initial one). */
int sfe_dsp_rs_load_history(sfe_rs_t h, const void *d_prev, size_t n_prev, size_t stride,
                            sfe_stream_t stream);
int sfe_dsp_rs_seek(sfe_rs_t h, uint64_t first_sample, float rate);
/* the host pipe (sfe_dsp_pipe_*) over a single-channel resample / decimate handle at `rate`: batches of whole
 * blksize-sample reference calls; items in are float32 samples, or u8 wire-format items when the handle's input
 * format is SFE_FMT_U8 (integer-valued steps); items out float32 */
int sfe_dsp_rs_pipe_create(sfe_rs_t rs, size_t batch_items, float rate, sfe_pipe_t *out);
int sfe_dsp_rs_reset(sfe_rs_t h);
int sfe_dsp_rs_destroy(sfe_rs_t h);
/* Channel groups of resample / decimate objects (one reference object per stream,
 * libdsp/resample.h:33-61, libdsp/decimate.h:33-63): the same partition, calls and guarantees as
 * sfe_dsp_fir_group_* above.  All blocks are fed in lockstep, so every channel produces the same
 * *n_out; a block handle driven on its own makes the next group call fail with SFE_ESTATE. */
typedef void *sfe_rs_group_t;
int sfe_dsp_rs_group_create(const float *taps, int n_taps, int upsample, int blksize, int data_complex, int n_channels,
                            const int *devices, int n_devices, int mode, sfe_rs_group_t *out);
int sfe_dsp_rs_group_shards(sfe_rs_group_t g, int *n_shards);
int sfe_dsp_rs_group_shard(sfe_rs_group_t g, int shard, int *device, int *first_channel, int *n_channels,
                           sfe_rs_t *handle, sfe_stream_t *stream);
int sfe_dsp_rs_group_process_stream(sfe_rs_group_t g, const void *const *d_in, size_t n_in, size_t in_stride,
                                    void *const *d_out, size_t out_cap, size_t out_stride, float rate, size_t *n_out);
int sfe_dsp_rs_group_sync(sfe_rs_group_t g);
int sfe_dsp_rs_group_reset(sfe_rs_group_t g);
int sfe_dsp_rs_group_destroy(sfe_rs_group_t g);

/* Host-only: replay the time law of ONE process() call without touching the GPU
 * (resample.cxx:89,119-150).  state = {pos, mu, leftover} in/out.  Writes up to cap
 * entries: rel_pos[k] = upsampled position of output k relative to the chunk start (-1 for
 * a leftover output), mu[k] its interpolation weight.  Returns the output count in *n_out. */
typedef struct {
    int32_t pos;
    float   mu;
    int32_t leftover;
} sfe_rs_timestate;
int sfe_dsp_rs_plan(sfe_rs_timestate *state, int upsample, int n_in, int out_len, float rate,
                    int32_t *rel_pos, float *mu, int cap, int *n_out);
/* The handle's time state (m_pos, m_mu, m_is_leftover: libdsp/resample.h:55-59), read / written
 * between calls: lets a stream be cut at ANY rate by carrying one span's final state to the next. */
/* Host-only form of sfe_dsp_rs_seek (no handle, no GPU): the state after `first_sample` samples. */
int sfe_dsp_rs_plan_seek(sfe_rs_timestate *state, int upsample, uint64_t first_sample, float rate);
int sfe_dsp_rs_get_state(sfe_rs_t h, sfe_rs_timestate *state);
int sfe_dsp_rs_set_state(sfe_rs_t h, const sfe_rs_timestate *state);

/* ------------------------------------------- wire-format converters ("next" row N2)
 * RX: u8 offset-binary -> float32 (b-128)*(1/127)
 *     gr-simplefe/lib/source_c_impl.cc:121-132, source_f_impl.cc:120-129.
 * TX: float32 -> 10-bit offset binary ((short)(x*511)+512)&0x3FF, 4 samples in 5 bytes
 *     gr-simplefe/lib/sink_c_impl.cc:118-144, sink_f_impl.cc:117-143,
 *     examples/bpsk/bpsk.cxx:76-101.   Device pointers, asynchronous. */
int sfe_dsp_rx_u8_to_f32(const void *d_bytes, void *d_floats, size_t n_bytes, sfe_stream_t stream);
int sfe_dsp_tx_f32_to_10bit(const void *d_floats, void *d_bytes, size_t n_floats, sfe_stream_t stream);

/* ------------------------------------------------- polyphase filter-bank channelizer
 * Splits a complex stream into M sub-bands in one pass over it (no reference counterpart: the
 * first step of a receive chain behind gr-simplefe's source, source_c_impl.cc:121-132).  With a
 * real prototype low-pass h[0..L), channel k (0 <= k < M) of output instant m is
 *     y_k[m] = sum_{n<L} h[n] x[mD - n] exp(-j 2 pi k (mD - n) / M)
 * x shifted down by k/M cycles per sample, filtered by h, every D-th sample kept: a true baseband
 * signal (channels k >= M/2 are the negative frequencies), no 1/M factor.  x[i] = 0 before the
 * first sample after create / reset.  Shapes: M a power of two in [4, 1024], D = M (critically
 * sampled) or M/2 (2x oversampled), 1 <= n_taps <= 32 M; anything else is SFE_EINVAL.
 * Computed by csrc/chan.hip: branch sums in registers, one M-point transform per instant in LDS. */
typedef void *sfe_chan_t;     /* opaque: one channelizer over n_streams streams */
/* Host-only (no GPU): validates the shape; *taps_per_branch = P = ceil(n_taps / M), *history =
 * the samples of carried state per stream the device keeps (>= n_taps - 1: whole tap chunks of
 * the kernel).  Either output pointer may be NULL. */
int sfe_dsp_chan_plan(int n_taps, int n_chans, int decim, int *taps_per_branch, int *history);
/*   taps       n_taps real float32 (copied, zero-padded to whole branches)
 *   n_chans    M;  decim  D
 *   n_streams  independent input streams sharing the taps, each with its own history and output
 *              counter.  SFE_ENODEV without a GPU: nothing computes on the CPU. */
int sfe_dsp_chan_create(const float *taps, int n_taps, int n_chans, int decim, int n_streams,
                        int device, sfe_chan_t *out);
/* SFE_FMT_F32 (cf32 input, 8-byte aligned) or SFE_FMT_U8 ((I,Q) byte pairs, 2-byte aligned,
 * converted (b-128)*(1/127) on load exactly as sfe_dsp_rx_u8_to_f32).  The carried state is kept
 * as cf32, so the format may change between calls. */
int sfe_dsp_chan_set_input_format(sfe_chan_t h, int fmt);
/* n_in samples of every stream: stream s at d_in + s*in_stride (samples of the input format);
 * channel k of stream s at d_out + (s*M + k)*out_stride (cf32 samples, 8-byte aligned).  n_in a
 * multiple of D (else SFE_EINVAL); *n_out = n_in / D per channel; n_in = 0 is a no-op.
 * out_stride < *n_out is SFE_ERANGE; overlapping input and output byte ranges, misaligned
 * buffers and in_stride < n_in with more than one stream are SFE_EINVAL; nothing is launched on
 * a refusal.  Cutting a stream into calls at any multiple of D gives the one-call result bit for
 * bit.  Asynchronous on `stream`, no host synchronisation or allocation.  The output counter
 * lives on the host: a call on a stream under graph capture is SFE_ESTATE, nothing enqueued. */
/* A stride that takes a buffer's byte range to 2^62 is SFE_EINVAL too; nothing is launched. */
int sfe_dsp_chan_process_stream(sfe_chan_t h, const void *d_in, size_t n_in, size_t in_stride,
                                void *d_out, size_t out_stride, size_t *n_out, sfe_stream_t stream);
/* Zero the carried state and the output counter (a fresh handle). */
int sfe_dsp_chan_reset(sfe_chan_t h);
int sfe_dsp_chan_destroy(sfe_chan_t h);

/* ------------------------------------------------- polyphase synthesis filter bank (combiner)
 * The transpose of the channelizer: M baseband channels at rate 1/D, each interpolated by D,
 * shifted up to its own sub-band and summed into one complex stream, in one pass.  With a real
 * prototype low-pass g[0..L) and channel inputs X_k[m] (k < M; m the absolute instant since
 * create / reset; X = 0 before the first instant), output sample i (absolute) is
 *     z[i] = sum_{m : 0 <= i - mD < L}  g[i - mD] * sum_{k<M} X_k[m] exp(+j 2 pi k i / M)
 * channel k zero-stuffed by D, filtered by g and shifted up by k/M cycles per sample (channels
 * k >= M/2 are the negative frequencies, numbered as the channelizer numbers them), no 1/M
 * factor.  Causal: a call over instants [m0, m0 + n) emits exactly the n D samples
 * [m0 D, (m0 + n) D), each complete.  Shapes: M a power of two in [4, 1024], D = M or M/2,
 * 1 <= n_taps <= 32 M; anything else is SFE_EINVAL.  The channelizer (D = M/2, h =
 * lowpass(16M+1, 2/M)) followed by this combiner (D = M/2, g = lowpass(16M+1, 1/M)) gives the
 * input back delayed by 16 M samples, times about 2/M.
 * Computed by csrc/combine.hip: one M-point transform per instant in LDS, the output FIR in
 * registers. */
typedef void *sfe_combine_t;  /* opaque: one combiner over n_streams output streams */
/* Host-only (no GPU): validates the shape; *taps_per_branch = P = ceil(n_taps / D) (taps per
 * output phase), *history = the instants of carried state per stream the device keeps (>= P - 1:
 * the kernel's delay line).  Either output pointer may be NULL. */
int sfe_dsp_combine_plan(int n_taps, int n_chans, int interp, int *taps_per_branch, int *history);
/*   taps       n_taps real float32 (copied, zero-padded to whole output phases)
 *   n_chans    M;  interp  D
 *   n_streams  independent streams sharing the taps, each with its own history and instant
 *              counter.  SFE_ENODEV without a GPU: nothing computes on the CPU. */
int sfe_dsp_combine_create(const float *taps, int n_taps, int n_chans, int interp, int n_streams,
                           int device, sfe_combine_t *out);
/* SFE_FMT_F32 (cf32 output, 8-byte aligned) or SFE_FMT_TX10 (the transmit wire format written by
 * the same launch: 4 floats, i.e. 2 complex samples, in 5 bytes, the bits of
 * sfe_dsp_tx_f32_to_10bit on the F32 output; stream s at byte d_out + s*(out_stride/2)*5, (n_out/2)*5
 * bytes, no alignment needed; out_stride must be even). */
int sfe_dsp_combine_set_output_format(sfe_combine_t h, int fmt);
/* n_in instants of every channel of every stream: channel k of stream s at d_in + (s*M + k)*in_stride
 * (cf32 samples, 8-byte aligned -- the channelizer's output layout); stream s's output at
 * d_out + s*out_stride samples.  *n_out = n_in * D per stream; n_in = 0 is a no-op.
 * out_stride < *n_out is SFE_ERANGE; in_stride < n_in, misaligned buffers, overlapping input and
 * output byte ranges, an odd out_stride under SFE_FMT_TX10, or a stream whose input or output
 * reaches 2^31 samples are SFE_EINVAL; nothing is launched on a refusal.  Cutting a stream into
 * calls at any instant gives the one-call result bit for bit.  Asynchronous on `stream`, no host
 * synchronisation or allocation.  The instant counter lives on the host: a call on a stream under
 * graph capture is SFE_ESTATE, nothing enqueued. */
/* A stride that takes a buffer's byte range to 2^62 is SFE_EINVAL too; nothing is launched. */
int sfe_dsp_combine_process_stream(sfe_combine_t h, const void *d_in, size_t n_in, size_t in_stride,
                                   void *d_out, size_t out_stride, size_t *n_out, sfe_stream_t stream);
/* Zero the carried state and the instant counter (a fresh handle). */
int sfe_dsp_combine_reset(sfe_combine_t h);
int sfe_dsp_combine_destroy(sfe_combine_t h);

/* ------------------------------------------------- digital down-converter bank
 * K tunings of one stream, each shifted to baseband at its own frequency, low-pass filtered by
 * one real prototype h[0..L) and decimated by any integer D, from one pass over the input (the
 * frequency-translating FIR, K at a time).  Each frequency f_k in [-0.5, 0.5] cycles per sample
 * is quantised to a 32-bit NCO increment inc_k = llround(f_k 2^32) mod 2^32 (NaN or any other
 * value is SFE_EINVAL).  With i the absolute input index since create / reset (x = 0 before it):
 *     phi_k(i) = (i inc_k) mod 2^32
 *     y_k[m]   = sum_{n<L} h[n] x[mD - n] exp(-j 2 pi phi_k(mD - n) / 2^32)
 * a true baseband signal, no 1/D factor.  Shapes: 1 <= D <= 1024, 1 <= L <= 8192 with
 * P = ceil(L/D) <= 64, 1 <= K <= 64; anything else is SFE_EINVAL.  Input: complex (cf32, or u8
 * (I,Q) pairs) or real float32; the output is always cf32.
 * Computed by csrc/ddc.hip: the taps are rotated per tuning on the host (g_k[n] = h[n]
 * exp(+j 2 pi phi_k(n) / 2^32)), the kernel is one complex-tap decimating FIR over the shared
 * input samples, and each output is multiplied by exp(-j 2 pi phi_k(mD) / 2^32). */
typedef void *sfe_ddc_t;  /* opaque: one down-converter bank over n_streams input streams */
/* Host-only (no GPU): validates the shape and the frequencies; *taps_per_branch = P,
 * *history = the samples of carried state per stream the device keeps (>= L - 1: whole tap
 * chunks of the kernel), phase_inc[0..K) = the quantised increments.  Any output pointer may be
 * NULL. */
int sfe_dsp_ddc_plan(int n_taps, int decim, int n_tunings, const double *freqs,
                     int *taps_per_branch, int *history, uint32_t *phase_inc);
/*   taps          n_taps real float32 (copied)
 *   decim         D;  n_tunings  K;  freqs  K frequencies in cycles per sample
 *   data_complex  1: complex input (cf32, or u8 with sfe_dsp_ddc_set_input_format), 0: real float32
 *   n_streams     independent streams sharing the taps and tunings, each with its own history
 *                 and sample counter.  SFE_ENODEV without a GPU: nothing computes on the CPU. */
int sfe_dsp_ddc_create(const float *taps, int n_taps, int decim, int n_tunings, const double *freqs,
                       int data_complex, int n_streams, int device, sfe_ddc_t *out);
/* SFE_FMT_F32 (cf32 input, 8-byte aligned; real float32, 4-byte aligned, for a real handle) or
 * SFE_FMT_U8 ((I,Q) byte pairs, 2-byte aligned, converted (b-128)*(1/127) on load exactly as
 * sfe_dsp_rx_u8_to_f32; complex handles only, SFE_EINVAL on a real one).  The carried state of a
 * complex handle is kept as cf32, so the format may change between calls; u8 input gives the
 * bits of the cf32 path on the converted samples. */
int sfe_dsp_ddc_set_input_format(sfe_ddc_t h, int fmt);
/* K new frequencies (validated as in create), used over the whole window of every output of
 * every later call: from the first output of the next call on, the result equals, bit for bit,
 * a fresh handle created with the new frequencies and fed the whole stream.  There is NO phase
 * continuity across a retune: each output's phase is that of its absolute sample index under
 * the new increments.  May block until the handle's earlier calls have finished; never changes
 * what an already-enqueued call computes. */
int sfe_dsp_ddc_set_freqs(sfe_ddc_t h, const double *freqs);
/* n_in samples of every stream: stream s at d_in + s*in_stride (samples of the input format);
 * tuning k of stream s at d_out + (s*K + k)*out_stride (cf32 samples, 8-byte aligned).  n_in a
 * multiple of D below 2^31 (else SFE_EINVAL); *n_out = n_in / D per tuning; n_in = 0 is a no-op.
 * out_stride < *n_out is SFE_ERANGE; overlapping input and output byte ranges, misaligned
 * buffers and in_stride < n_in with more than one stream are SFE_EINVAL; nothing is launched on
 * a refusal.  Cutting a stream into calls at any multiple of D gives the one-call result bit for
 * bit.  Asynchronous on `stream`, no host synchronisation or allocation.  The sample counter
 * lives on the host: a call on a stream under graph capture is SFE_ESTATE, nothing enqueued. */
/* A stride that takes a buffer's byte range to 2^62 is SFE_EINVAL too; nothing is launched. */
int sfe_dsp_ddc_process_stream(sfe_ddc_t h, const void *d_in, size_t n_in, size_t in_stride,
                               void *d_out, size_t out_stride, size_t *n_out, sfe_stream_t stream);
/* Zero the carried state and the sample counter; the tunings are kept. */
int sfe_dsp_ddc_reset(sfe_ddc_t h);
int sfe_dsp_ddc_destroy(sfe_ddc_t h);

/* ------------------------------------------------- streaming Welch spectrum estimator
 * Averaged, windowed periodograms of complex streams, every stream in one kernel pass per call:
 * what is in this band, before anything is tuned to it.  With a real window w[0..N), a hop H, an
 * averaging count A and a float32 scale; i the absolute sample index since create / reset
 * (x[i] = 0 for i < 0) and m >= 0 the absolute segment index:
 *     b_m      = (m + 1) H - N                      first sample of segment m
 *     X_m[k]   = sum_{n<N} w[n] x[b_m + n] exp(-j 2 pi k n / N)
 *     P_m[k]   = Re(X_m[k])^2 + Im(X_m[k])^2
 *     out_r[k] = scale * S_r[k],   S_r = the sum of P_m over m in [rA, (r + 1)A)
 * Bin k is frequency k/N cycles per sample (bins k >= N/2 are the negative frequencies, numbered
 * as the channelizer numbers them).  No implicit normalisation: the caller puts 1 / (A sum w^2),
 * or whatever it wants, into scale.  Causal like the channelizer: a call of n_in = q H samples
 * completes exactly q segments, and every emitted value is complete.
 * Summation order (part of the contract: any cut of the stream gives the same bits).  A row's
 * segments are taken in chunks of C consecutive segments counted from the row's first one (the
 * last chunk of a row may be shorter); a chunk sum is the float32 left fold, from 0, of its P_m
 * in ascending m; S_r is the float32 left fold, from 0, of its chunk sums in ascending order;
 * scale multiplies once, after the last fold.  C is the smallest power of two with C C >= A
 * (sfe_dsp_psd_plan reports it).  The order is a function of (A, m - rA) only: never of where
 * calls are cut, of the grid size, or of the input format.  Every fold is about 2 sqrt(A) deep at
 * the most, and a one-row average over a whole capture is still sqrt(A) workgroups wide.
 * Shapes: N a power of two in [256, 4096], 1 <= H <= N (any integer), 1 <= A <= 2^24, scale
 * finite, n_streams >= 1; anything else is SFE_EINVAL.  There is no flush: an unfinished row is
 * dropped by reset; for one Welch estimate of a capture set A to its segment count.
 * Computed by csrc/psd.hip: windowed segments transformed in LDS, squared and folded in
 * registers per chunk; a second small kernel folds the chunk sums per row. */
typedef void *sfe_psd_t;  /* opaque: one estimator over n_streams streams */
/* Host-only (no GPU): validates the shape; *chunk = C, *history = N - H, the samples of carried
 * state per stream.  Either output pointer may be NULL. */
int sfe_dsp_psd_plan(int n_fft, int hop, int n_avg, int *chunk, int *history);
/*   window     n_fft real float32 (copied)
 *   hop        H;  n_avg  A;  scale  multiplies every row once
 *   n_streams  independent streams sharing the window, each with its own history, open chunk and
 *              open row; one segment counter.  SFE_ENODEV without a GPU: nothing computes on the CPU. */
int sfe_dsp_psd_create(const float *window, int n_fft, int hop, int n_avg, float scale,
                       int n_streams, int device, sfe_psd_t *out);
/* SFE_FMT_F32 (cf32 input, 8-byte aligned) or SFE_FMT_U8 ((I,Q) byte pairs, 2-byte aligned,
 * converted (b-128)*(1/127) on load exactly as sfe_dsp_rx_u8_to_f32).  The carried history is kept
 * as cf32, so the format may change between calls; u8 input gives the bits of the cf32 path on
 * the converted samples, and any element-aligned buffer gives the same bits. */
int sfe_dsp_psd_set_input_format(sfe_psd_t h, int fmt);
/* n_in samples of every stream: stream s at d_in + s*in_stride (samples of the input format).
 * The rows this call completes are written consecutively: row j of stream s at
 * d_out + s*out_stride + j*N (float32, 4-byte aligned); *n_rows = floor((segments_before mod A +
 * n_in/H) / A).  A call that completes no row writes nothing and returns SFE_OK with *n_rows = 0.
 * n_in a multiple of H below 2^31 (else SFE_EINVAL); n_in = 0 is a no-op.  out_stride <
 * *n_rows * N is SFE_ERANGE; null or misaligned buffers, in_stride < n_in with more than one
 * stream and overlapping input and output byte ranges are SFE_EINVAL; nothing is launched on a
 * refusal.  Cutting a stream into calls at any multiple of H gives the one-call rows bit for bit,
 * cuts in mid-chunk and mid-row included.  Asynchronous on `stream`.  The handle owns a scratch
 * buffer for the chunk sums of one call, sized on the first call and grown only when a larger
 * call arrives (synchronise, free, allocate): that is the one allocation, and the one host
 * synchronisation, a call may make.  The segment counter lives on the host: a call on a stream
 * under graph capture is SFE_ESTATE, nothing enqueued. */
/* A stride that takes a buffer's byte range to 2^62 is SFE_EINVAL too; nothing is launched. */
int sfe_dsp_psd_process_stream(sfe_psd_t h, const void *d_in, size_t n_in, size_t in_stride,
                               void *d_out, size_t out_stride, size_t *n_rows, sfe_stream_t stream);
/* Zero the carried state and the segment counter (a fresh handle); an unfinished row is dropped. */
int sfe_dsp_psd_reset(sfe_psd_t h);
int sfe_dsp_psd_destroy(sfe_psd_t h);

/* ------------------------------------------------- streaming preamble correlator bank
 * Where in a stream a known waveform starts: K complex templates s_k[0..L) against every stream,
 * normalised by the sliding signal energy and reduced to one peak per block on the chip, so a call
 * reads its input once, whatever K is, and writes 8 bytes per template and block.  With i the
 * absolute sample index since create / reset (x[i] = 0 for i < 0):
 *     c_k[i] = sum_{n<L} conj(s_k[n]) x[i - (L-1) + n]      window ENDING at sample i (causal)
 *     e[i]   = sum_{n<L} |x[i - (L-1) + n]|^2
 *     E_k    = sum_n |s_k[n]|^2       (host, float64, rounded once to float32; 0 is SFE_EINVAL)
 *     m_k[i] = |c_k[i]|^2 / (E_k e[i])   if e[i] > min_energy,   else 0
 * m is the squared normalised correlation: in [0, 1] up to rounding, not clamped, 1 where the
 * window is a multiple of the template.  Block j is the samples [jB, (j+1)B); per stream, template
 * and block the call emits peak_val = the maximum of m_k over the block and peak_idx = the smallest
 * offset i - jB that attains it (uint32).  The template whose peak this is began at sample
 * jB + peak_idx - (L-1).  Optionally m_k[i] of every sample is written too (the dense output).
 * Shapes: 1 <= L <= 2049, 1 <= K <= 16, n_streams >= 1, min_energy finite and >= 0, B a positive
 * multiple of the transform advance V(L) = 4096 - 256 ceil((L-1)/256) (sfe_dsp_fir_plan's rule for a
 * single partition: 4096 for L = 1, 3840 for L <= 257, 2048 at L = 2049); anything else is
 * SFE_EINVAL with a message that starts with "corr: ".
 * Computed by overlap-save through 4096-point transforms whose slots start at absolute multiples
 * of V, so every value is a function of absolute position only:
 *   - cutting the stream into calls at any multiple of B gives the one-call bits, peaks and dense;
 *   - u8 input gives the bits of the cf32 path on the converted samples, and the format may change
 *     between calls (the carried history, 4096 - V samples per stream, is cf32);
 *   - stream s of an n-stream handle gives the bits of a one-stream handle fed that stream, and
 *     template k of a K-template handle those of a one-template handle holding s_k;
 *   - the peaks are the same bits with and without the dense output, and equal the maximum and the
 *     first arg-maximum of the dense values of their block exactly.
 * e[i] is summed from the squares themselves (runs of 1, 16 and 256 samples in an order fixed by
 * the window's place in its slot), never as a difference of prefix sums.  The transform's rounding
 * error in c is relative to the RMS of the whole 4096-sample slot, not of the window: in a slot
 * that holds a strong burst and near-silence, m over the silence is noise divided by a tiny e, and
 * min_energy is the gate for that.  Non-finite samples poison the slots they touch. */
typedef void *sfe_corr_t;  /* opaque: one bank of K templates over n_streams streams */
/* Host-only (no GPU): validates what create validates except the template values;
 * *advance = V(L), *history = 4096 - V.  Either output pointer may be NULL. */
int sfe_dsp_corr_plan(int len, int n_templates, int block, int *advance, int *history);
/*   templates  [n_templates][len] complex float32 as (re, im) pairs (copied; their spectra are
 *              computed here, in float64)
 *   block      B;  min_energy  the gate on e[i]
 *   n_streams  independent streams sharing the templates, each with its own history.
 * Shapes and template values are checked before the device: SFE_ENODEV without a GPU. */
int sfe_dsp_corr_create(const float *templates, int len, int n_templates, int block,
                        float min_energy, int n_streams, int device, sfe_corr_t *out);
/* SFE_FMT_F32 (cf32 input, 8-byte aligned) or SFE_FMT_U8 ((I,Q) byte pairs, 2-byte aligned,
 * converted (b-128)*(1/127) on load exactly as sfe_dsp_rx_u8_to_f32). */
int sfe_dsp_corr_set_input_format(sfe_corr_t h, int fmt);
/* n_in samples of every stream: stream s at d_in + s*in_stride (samples of the input format).
 * Block j of template k of stream s goes to element (s*K + k)*peak_stride + j of d_peak_val
 * (float32) and of d_peak_idx (uint32), both 4-byte aligned; with d_metric != NULL, m_k of the
 * call's sample i goes to element (s*K + k)*metric_stride + i of d_metric (float32).
 * *n_blocks = n_in / B.  n_in a multiple of B below 2^31 (else SFE_EINVAL); n_in = 0 is a no-op.
 * peak_stride < *n_blocks, or metric_stride < n_in with a dense pointer, is SFE_ERANGE; null or
 * misaligned buffers, in_stride < n_in with more than one stream and any overlap between the
 * input and an output byte range (or between two outputs) are SFE_EINVAL; nothing is launched on
 * a refusal.  Asynchronous on `stream`.  With B = V a call allocates nothing; with B > V the handle
 * owns a table of one peak per 4096-point slot of a call, sized on the first call and grown only
 * when a larger call arrives (synchronise, free, allocate): the one allocation, and the one host
 * synchronisation, a call may make.  The sample counter lives on the host: a call on a stream
 * under graph capture is SFE_ESTATE, nothing enqueued. */
/* A stride that takes a buffer's byte range to 2^62 is SFE_EINVAL too; nothing is launched. */
int sfe_dsp_corr_process_stream(sfe_corr_t h, const void *d_in, size_t n_in, size_t in_stride,
                                void *d_peak_val, void *d_peak_idx, size_t peak_stride,
                                void *d_metric, size_t metric_stride,
                                size_t *n_blocks, sfe_stream_t stream);
/* Zero the carried history and the sample counter (a fresh handle); the templates are kept. */
int sfe_dsp_corr_reset(sfe_corr_t h);
int sfe_dsp_corr_destroy(sfe_corr_t h);

/* ------------------------------------------------- streaming biquad-cascade IIR filter
 * A recursive filter over every stream: S second-order sections in cascade, 1 <= S <= 8.  What no
 * finite window reaches at a bearable length: a DC blocker at pole radius 0.9999, a narrow notch,
 * a one-pole smoother, a steep low-pass.
 * Coefficients come as const double sos[S][6], one row (b0, b1, b2, a0, a1, a2) per section
 * (scipy's sos layout; a first-order section has b2 = a2 = 0).  The host divides each row by a0 in
 * float64 and rounds each of B0, B1, B2, A1, A2 ONCE to float32; the law is stated on those
 * float32 values promoted to real numbers.  With i the absolute sample index since create / reset
 * and everything 0 for i < 0:
 *     v_0 = x
 *     v_{s+1}[i] = B0_s v_s[i] + B1_s v_s[i-1] + B2_s v_s[i-2] - A1_s v_{s+1}[i-1] - A2_s v_{s+1}[i-2]
 *     y = v_S
 * The coefficients are real: on a complex stream I and Q never mix.
 * Refused with SFE_EINVAL and a message that starts with "iir: ": S outside [1, 8]; any of the 6S
 * numbers non-finite; a0 = 0; a section that is not strictly stable AS THE KERNEL WILL RUN IT, the
 * test being on the rounded values: |A2| < 1 and |A1| < 1 + A2.
 * Input: cf32; u8 (I,Q) pairs, converted exactly as sfe_dsp_rx_u8_to_f32 converts them; or, on a
 * handle created with data_complex = 0, real float32.  Output: cf32, or real float32 for a real
 * handle; one output sample per input sample.  A non-finite sample poisons its stream until reset
 * (the carried state is then non-finite, and so is every later output).
 * Computed exactly in parallel, not by warm-up and discard (csrc/iir.hip): a call is cut into
 * blocks of G samples, every block is run from zero state, the block states are chained from the
 * carried state (in two levels, grouped by the absolute block index since create / reset, never
 * by where calls are cut), and every block is run again from its true state.
 * Contracts about bits:
 *   1. cutting a stream into calls at any multiple of G gives the one-call output bit for bit;
 *   2. u8 input gives the bits of the cf32 path on the converted samples, at any 2-byte-aligned
 *      address, and the format may change between calls (the carried state is float32);
 *   3. stream s of an n-stream handle gives the bits of a one-stream handle fed that stream;
 *   4. a complex handle's output equals, bit for bit, two real handles run on its real and its
 *      imaginary parts;
 *   5. the same calls give the same bits on every run: nothing depends on the order in which
 *      workgroups finish, and there are no floating-point atomics;
 *   6. reset makes a fresh handle.
 * Not promised: the bits of the sample-by-sample float32 recursion (the error is of its size, see
 * DESIGN.md 4.10), nor equal bits between a cascade and the same sections run as separate handles. */
typedef void *sfe_iir_t;  /* opaque: one cascade over n_streams streams */
/* Host-only (no GPU): validates the coefficients as above; *block = G, the granule of a call (a
 * power of two in [1024, 65536], the same for every S and format); *state_floats = 6S, the float32
 * values of carried state per stream and component (a complex stream carries I's and Q's): the
 * 2S states of the cascade, and two more such vectors of the two-level fold over the blocks.
 * Either output pointer may be NULL. */
int sfe_dsp_iir_plan(const double *sos, int n_sections, int *block, int *state_floats);
/*   sos           [n_sections][6] float64 (copied after normalising and rounding)
 *   data_complex  0: real float32 streams; else complex
 *   n_streams     independent streams sharing the coefficients, each with its own state.
 * The coefficients are checked before the device: SFE_ENODEV without a GPU. */
int sfe_dsp_iir_create(const double *sos, int n_sections, int data_complex, int n_streams,
                       int device, sfe_iir_t *out);
/* SFE_FMT_F32 (cf32 input, 8-byte aligned; float32, 4-byte aligned, on a real handle) or
 * SFE_FMT_U8 ((I,Q) byte pairs, 2-byte aligned, converted (b-128)*(1/127) on load).  u8 on a real
 * handle and any other format are SFE_EINVAL. */
int sfe_dsp_iir_set_input_format(sfe_iir_t h, int fmt);
/* n_in samples of every stream: stream s at d_in + s*in_stride (samples of the input format) goes
 * to d_out + s*out_stride (samples of the output format).  *n_out = n_in.  n_in a positive
 * multiple of G below 2^31 (else SFE_EINVAL); n_in = 0 is a no-op.  out_stride < n_in is
 * SFE_ERANGE; null or misaligned buffers, overlapping input and output byte ranges and
 * in_stride < n_in with more than one stream are SFE_EINVAL; nothing is launched on a refusal.
 * Asynchronous on `stream`.  The handle owns one table of per-block states, sized on the first
 * call and grown only when a larger call arrives (synchronise, free, allocate): that is the one
 * allocation, and the one host synchronisation, a call may make.  The sample counter lives on the
 * host: a call on a stream under graph capture is SFE_ESTATE, nothing enqueued. */
/* A stride that takes a buffer's byte range to 2^62 is SFE_EINVAL too; nothing is launched. */
int sfe_dsp_iir_process_stream(sfe_iir_t h, const void *d_in, size_t n_in, size_t in_stride,
                               void *d_out, size_t out_stride, size_t *n_out, sfe_stream_t stream);
/* Zero the carried state and the sample counter (a fresh handle); the coefficients are kept. */
int sfe_dsp_iir_reset(sfe_iir_t h);
int sfe_dsp_iir_destroy(sfe_iir_t h);

/* ------------------------------------------------- multi-stream beamformer / stream-mixing bank
 * The one block whose streams meet: B output beams out of S input streams, in each of M bands
 * (M = 1: narrowband).  Band k holds complex weights W_k[b][s] and, optionally, conjugate weights
 * V_k[b][s] (absent: all zero), and
 *     y_{b,k}[m] = sum_{s<S}  W_k[b][s] x_{s,k}[m]  +  V_k[b][s] conj(x_{s,k}[m])
 * -- a beam, a null, a diversity combiner, a sub-band mix; with S = B = 1 and V the I/Q imbalance
 * correction y = a x + b conj(x) of a direct-conversion receiver.
 * Real matrix.  The host turns each band's (W, V) into one real matrix R_k of 2B x 2S float32:
 * row 2b is Re y_b, row 2b+1 is Im y_b, column 2s is Re x_s, column 2s+1 is Im x_s, and
 *     R[2b][2s]   =  Wr + Vr        R[2b][2s+1]   = -Wi + Vi
 *     R[2b+1][2s] =  Wi + Vi        R[2b+1][2s+1] =  Wr - Vr
 * each entry formed in float64 from the float32 arguments and rounded ONCE to float32; with V
 * absent the entries are W's own floats, up to sign.  The law is stated on those rounded values:
 * each output float is a float32 dot product of length 2S, computed on the matrix pipe
 * (csrc/beam.hip) as a chain of fused multiply-adds from zero.  The order of the 2S terms is
 * fixed per shape (S, B); it never depends on where a sample sits in a call, a tile or a buffer.
 * Layouts.  There is no state across samples: no carried history and NO GRANULE, any n_in >= 1 is
 * accepted.  x_{s,k}[m] is at d_in + (s*M + k)*in_stride + m (sfe_dsp_chan_*'s output layout);
 * y_{b,k}[m] is at d_out + (b*M + k)*out_stride + m (sfe_dsp_combine_*'s input layout), cf32,
 * 8-byte aligned.  Input: cf32 (8-byte aligned) or SFE_FMT_U8 (I,Q) byte pairs (2-byte aligned),
 * converted (b-128)*(1/127) on load exactly as sfe_dsp_rx_u8_to_f32 converts them.  A non-finite
 * input sample poisons every beam of its own instant and band (0 * NaN is NaN) and nothing else.
 * Shapes: 1 <= S <= 64, 1 <= B <= 64, 1 <= M <= 1024, M*B*S <= 2^20, every weight finite;
 * anything else is SFE_EINVAL with a message that starts with "beam: ".
 * Contracts about bits:
 *   1. cutting a stream into calls at ANY sample gives the one-call output bit for bit, and so does
 *      moving a buffer to any element-aligned address or changing the strides (a call's tail runs
 *      the arithmetic of its body, with masked loads and stores);
 *   2. u8 input gives the bits of the cf32 path on the converted samples, and the format may
 *      change between calls;
 *   3. band k of an M-band handle gives the bits of a one-band handle of the same (S, B) holding
 *      W_k, V_k;
 *   4. a selection is exact: if each row of W has a single entry 1+0j, the rest 0 and V absent,
 *      beam b is the chosen stream bit for bit on finite input; with that entry placed in V
 *      instead, it is the stream's conjugate bit for bit (a zero comes out as +0: a sum that
 *      starts from zero cannot return -0);
 *   5. the same calls give the same bits on every run.
 * Not promised: equal bits between different shapes (S, B) -- beam b of a 64-beam handle may
 * differ in the last place from a one-beam handle holding row b -- nor the bits of any particular
 * left fold. */
typedef void *sfe_beam_t; /* opaque: one weight set, M bands of S streams into B beams */
/* Host-only (no GPU): validates the shape and the weights as above; if real_matrix != NULL writes
 * the M*2B*2S float32 of the R_k there, band-major, each row-major.
 *   weights       [n_bands][n_beams][n_in] (re, im) float32 pairs
 *   weights_conj  the same shape, or NULL */
int sfe_dsp_beam_plan(int n_in, int n_beams, int n_bands, const float *weights,
                      const float *weights_conj, float *real_matrix);
/* The weights are copied.  Shapes and weight values are checked before the device is touched:
 * SFE_EINVAL for a bad shape on any machine, SFE_ENODEV without a GPU. */
int sfe_dsp_beam_create(const float *weights, const float *weights_conj, int n_in, int n_beams,
                        int n_bands, int device, sfe_beam_t *out);
/* SFE_FMT_F32 (cf32 input, 8-byte aligned) or SFE_FMT_U8 ((I,Q) byte pairs, 2-byte aligned,
 * converted on load); any other format is SFE_EINVAL. */
int sfe_dsp_beam_set_input_format(sfe_beam_t h, int fmt);
/* New weights of the handle's shape (validated as at create), used from the next call on: the
 * result then equals a fresh handle created with them, bit for bit.  May block until the handle's
 * earlier calls have finished; never changes what an already enqueued call computes. */
int sfe_dsp_beam_set_weights(sfe_beam_t h, const float *weights, const float *weights_conj);
/* n_in samples of every band of every stream.  *n_out = n_in.  n_in = 0 is a no-op; n_in >= 2^31
 * is SFE_EINVAL.  out_stride < n_in is SFE_ERANGE; in_stride < n_in, null or misaligned buffers
 * and overlapping input and output byte ranges are SFE_EINVAL; nothing is launched on a refusal.
 * Asynchronous on `stream`; allocates nothing and does not synchronise the host.  A call on a
 * stream under graph capture is SFE_ESTATE, nothing enqueued: sfe_dsp_beam_set_weights may
 * replace the table a captured call would have pinned.
 * There is no reset: there is nothing to reset. */
/* A stride that takes a buffer's byte range to 2^62 is SFE_EINVAL too; nothing is launched. */
int sfe_dsp_beam_process_stream(sfe_beam_t h, const void *d_in, size_t n_in, size_t in_stride,
                                void *d_out, size_t out_stride, size_t *n_out, sfe_stream_t stream);
int sfe_dsp_beam_destroy(sfe_beam_t h);

/* ------------------------------------------------- streaming spatial covariance estimator
 * Where the beamformer's weights come from: the sample covariance of the S streams of each of M
 * bands, averaged A instants at a time.  Write instant m of band k as a real column of 2S floats,
 *     u[2s] = Re x_{s,k}[m],   u[2s+1] = Im x_{s,k}[m]
 * (interleaved cf32 as it lies in memory, and the beamformer's column order).  Output row r of band
 * k is the real Gram matrix
 *     G_r[i][j] = scale * sum over m in [rA, (r + 1)A) of u_i[m] u_j[m]
 * 2S x 2S float32, row-major, stored whole (both triangles); m the absolute instant since create /
 * reset.  One real matrix carries the covariance C = E[x x^H] and the pseudo-covariance
 * P = E[x x^T] that the beamformer's widely-linear weights V need:
 *     C[s][t] = (G[2s][2t] + G[2s+1][2t+1]) + j (G[2s+1][2t] - G[2s][2t+1])
 *     P[s][t] = (G[2s][2t] - G[2s+1][2t+1]) + j (G[2s+1][2t] + G[2s][2t+1])
 * No implicit normalisation: the caller puts 1/A into scale.
 * Summation order (part of the contract).  A row's instants are taken in chunks of T consecutive
 * instants counted from the row's first; the chunk partial of entry (i, j) is the float32 fmaf
 * chain from +0 over its T products in ascending instant order (what consecutive
 * v_mfma_f32_16x16x4_f32 instructions compute when K is the instant index).  Chunks are taken in
 * groups of C consecutive chunks counted from the row's first (the last group of a row may be
 * shorter), C the smallest power of two with C C >= A/T; the group sum is the float32 left fold,
 * from 0, of its chunk partials in ascending order; the row is the float32 left fold, from 0, of
 * its group sums in ascending order; scale multiplies once, after the last fold.  T = 64 for every
 * S, M and format (sfe_dsp_cov_plan reports T and C).  The order is a function of (A, m - rA)
 * only: never of S, of where calls are cut, of the grid or of the input format.
 * Shapes: 1 <= S <= 64, 1 <= M <= 1024, A a positive multiple of T at most 2^24, scale finite;
 * anything else is SFE_EINVAL with a message that starts with "cov: ".
 * Layouts: x_{s,k}[m] is at d_in + (s*M + k)*in_stride + m (sfe_dsp_chan_*'s output layout and
 * sfe_dsp_beam_*'s input layout); cf32 (8-byte aligned) or SFE_FMT_U8 (I,Q) byte pairs (2-byte
 * aligned), converted (b-128)*(1/127) on load exactly as sfe_dsp_rx_u8_to_f32 converts them.
 * Contracts about bits:
 *   1. cutting a stream into calls at any multiple of T gives the one-call rows bit for bit, cuts
 *      in mid-group and mid-row included;
 *   2. u8 input gives the bits of the cf32 path on the converted samples, and the format may
 *      change between calls (the carried state is float32 sums, not samples);
 *   3. band k of an M-band handle gives the bits of a one-band handle fed band k;
 *   4. entry (i, j) depends on rows i and j of U only: a handle over any subset of the streams
 *      gives the same bits for the entries they share (S = 1 handles reproduce the 2 x 2 diagonal
 *      blocks of any larger handle);
 *   5. G[i][j] and G[j][i] are the same bits;
 *   6. small-integer cf32 input (every product and partial sum exact in float32) with scale a
 *      power of two gives the exact Gram;
 *   7. a non-finite sample poisons rows and columns 2s, 2s+1 of its own stream, in its own band
 *      and output row, and nothing else; the next output row is clean;
 *   8. the same calls give the same bits on every run;
 *   9. reset makes a fresh handle.
 * Not promised: the bits of any other fold (a plain left fold over A, a library matmul).
 * Computed by csrc/cov.hip: a chunk of U staged in LDS, the upper-triangular 16 x 16 tiles on the
 * f32 matrix pipe, chunk partial and group sum in registers; a second small kernel folds the
 * group sums per row and mirrors the triangle on the store. */
typedef void *sfe_cov_t;  /* opaque: one estimator over M bands of S streams */
/* Host-only (no GPU): validates the shape; *chunk = T, *group = C.  Either output pointer may be
 * NULL. */
int sfe_dsp_cov_plan(int n_in_streams, int n_bands, int n_avg, int *chunk, int *group);
/* Every band has its own open group and open row; one instant counter.  Shapes are checked before
 * the device is touched: SFE_EINVAL for a bad shape on any machine, SFE_ENODEV without a GPU. */
int sfe_dsp_cov_create(int n_in_streams, int n_bands, int n_avg, float scale, int device,
                       sfe_cov_t *out);
/* SFE_FMT_F32 (cf32 input, 8-byte aligned) or SFE_FMT_U8 ((I,Q) byte pairs, 2-byte aligned,
 * converted on load); any other format is SFE_EINVAL. */
int sfe_dsp_cov_set_input_format(sfe_cov_t h, int fmt);
/* n_in instants of every band of every stream.  The rows this call completes are written
 * consecutively: row j of band k at d_out + k*out_stride + j*(2S)^2 (float32, 4-byte aligned);
 * *n_rows = floor((instants_before mod A + n_in) / A).  A call that completes no row writes
 * nothing and returns SFE_OK with *n_rows = 0.  n_in a multiple of T below 2^31 (else
 * SFE_EINVAL); n_in = 0 is a no-op.  out_stride < *n_rows * (2S)^2 is SFE_ERANGE; in_stride <
 * n_in, null or misaligned buffers and overlapping input and output byte ranges are SFE_EINVAL;
 * nothing is launched on a refusal.  Asynchronous on `stream`.  The handle owns a scratch buffer
 * for the group sums of one call, sized on the first call and grown only when a larger call
 * arrives (synchronise, free, allocate): that is the one allocation, and the one host
 * synchronisation, a call may make.  The instant counter lives on the host: a call on a stream
 * under graph capture is SFE_ESTATE, nothing enqueued. */
/* A stride that takes a buffer's byte range to 2^62 is SFE_EINVAL too; nothing is launched. */
int sfe_dsp_cov_process_stream(sfe_cov_t h, const void *d_in, size_t n_in, size_t in_stride,
                               void *d_out, size_t out_stride, size_t *n_rows, sfe_stream_t stream);
/* Zero the carried state and the instant counter (a fresh handle); an unfinished row is dropped. */
int sfe_dsp_cov_reset(sfe_cov_t h);
int sfe_dsp_cov_destroy(sfe_cov_t h);

/* ------------------------------------------------- adaptive beamforming weight solver (MVDR)
 * The step between the covariance estimator and the beamformer, on the device: one regularised
 * minimum-variance distortionless-response problem per (output row j of sfe_dsp_cov_*, band k),
 * read where the estimator wrote it and written as the real matrix the beamformer multiplies by.
 * With the B steering vectors taken as scan directions the per-beam power is the Capon spectrum.
 * The law, on real matrices (n = 2S; G the n x n float32 Gram matrix; float32 on the device):
 *   1. Read.  Only G[i][j] with i <= j is read; the lower triangle is taken as its mirror
 *      (sfe_dsp_cov_* writes both with the same bits).
 *   2. Structure.  widely_linear = 1: G^ = G.  widely_linear = 0 (the covariance C alone, the
 *      pseudo-covariance ignored):
 *          G^[2s][2t]   =  G^[2s+1][2t+1] = (G[2s][2t] + G[2s+1][2t+1]) / 2
 *          G^[2s+1][2t] = -G^[2s][2t+1]   = (G[2s+1][2t] - G[2s][2t+1]) / 2
 *      (half the realification of C: trace G^ = trace G in both modes).
 *   3. Loading.  lambda = load_abs + load_rel * trace(G^) / n, G^[i][i] += lambda; in the linear
 *      mode that is the complex diagonal loading load_rel * tr(C) / S.
 *   4. Factor.  G^ = L L^T (Cholesky, no pivoting).  A pivot that is not finite or not > 0 fails
 *      the whole problem.
 *   5. Per beam b, a its steering vector (S complex values), u(a)[2s] = Re a_s, u(a)[2s+1] = Im a_s:
 *      linear:  z = G^^-1 u(a), q = u(a)^T z; row 2b of R is z / q and row 2b+1 its rotation,
 *          R[2b+1][2s] = -R[2b][2s+1],  R[2b+1][2s+1] = R[2b][2s]
 *      -- exactly the matrix of a complex W with V absent (sfe_dsp_beam_plan) -- and
 *      power_b = 2 / q = 1 / (a^H C_lambda^-1 a).
 *      widely linear:  A2 = [u(a), u(ja)] (n x 2), Z = G^^-1 A2, Q = A2^T Z (2 x 2, Q[0][1] used
 *      for both off-diagonal entries); rows 2b, 2b+1 of R are Q^-1 Z^T by the explicit 2 x 2
 *      inverse and power_b = trace(Q^-1).  (S = 1: A2 is square, so the constraint alone fixes
 *      R = A2^-1 -- the conventional beamformer of step 6, whatever G is -- and
 *      power_b = trace(G^) / |a|^2; that closed form is what is computed, not the cancellation
 *      the general formula would reach it through.)
 *      A q or det Q that is not finite or not > 0 fails that beam.  In both modes R_b A2 = I_2
 *      (unit response on the steering vector) at minimum output power.
 *   6. Failure never produces a NaN weight: a failed beam gets the conventional beamformer
 *      W = conj(a) / |a|^2, V = 0 -- formed on the host in float64 at create / set_steering,
 *      rounded once and kept on the device, so its bits are defined -- and a quiet NaN power.
 *      status of a problem: 0 all good, 1 the factorisation failed (every beam fell back), 2 the
 *      factorisation succeeded and at least one beam fell back.
 * Layouts.  Input: row j of band k at d_gram + k*in_stride + j*(2S)^2 floats (sfe_dsp_cov_*'s
 * output layout; in_stride is its out_stride).  Output: R of row j, band k at
 * d_real_matrix + j*out_stride + k*4BS; one row's block is [M][2B][2S], the layout of
 * sfe_dsp_beam_plan's real_matrix.  power (float32, optional) at d_power + j*power_stride + k*B + b;
 * status (int32, optional) at d_status + j*status_stride + k.  All 4-byte aligned.
 * Shapes: 1 <= S <= 64, 1 <= B <= 64, 1 <= M <= 1024, M*B*S <= 2^20 (the beamformer's), every
 * steering value finite and every steering vector non-zero, load_rel and load_abs finite and
 * >= 0, widely_linear 0 or 1; anything else is SFE_EINVAL with a message that starts with
 * "mvdr: ".
 * Contracts about bits:
 *   1. the same calls give the same bits on every run;
 *   2. a problem's output depends on its own G, its band's steering and the loading only: never
 *      on M, n_rows, j, addresses or strides; band k of an M-band handle gives the bits of a
 *      one-band handle holding band k's steering;
 *   3. beam b's two rows, its power and its fallback depend on a_b only: a B-beam handle
 *      reproduces B one-beam handles;
 *   4. in the linear mode R has the exact W-only structure of step 5;
 *   5. nothing of the strict lower triangle of G is read;
 *   6. a failed problem or beam gets the exact fallback bits and its status, its neighbours are
 *      untouched;
 *   7. nothing outside the rows written is touched.
 * Not promised: the bits of the host plan or of LAPACK, equal bits between different S, equal
 * bits under a permutation of the streams.
 * Computed by csrc/mvdr.hip: one workgroup per problem, the loaded matrix factored in LDS as a
 * packed triangle, the right-hand sides substituted eight lanes apiece. */
typedef void *sfe_mvdr_t; /* opaque: M bands of B steering vectors over S streams, a mode, a loading */
/* Host-only (no GPU): validates the arguments as above.  If gram != NULL it solves ONE row -- M
 * matrices [M][2S][2S], band-major -- by the law in float64 and rounds once to float32 into
 * real_matrix [M][2B][2S], power [M][B] and status [M], each of which may be NULL: the CPU
 * fallback, and the reference of the device's values (not of its bits).
 *   steering  [n_bands][n_beams][n_in] (re, im) float32 pairs */
int sfe_dsp_mvdr_plan(int n_in, int n_beams, int n_bands, const float *steering, int widely_linear,
                      float load_rel, float load_abs, const float *gram, float *real_matrix,
                      float *power, int *status);
/* The steering vectors are copied.  Arguments are checked before the device is touched:
 * SFE_EINVAL for a bad one on any machine, SFE_ENODEV without a GPU. */
int sfe_dsp_mvdr_create(const float *steering, int n_in, int n_beams, int n_bands,
                        int widely_linear, float load_rel, float load_abs, int device,
                        sfe_mvdr_t *out);
/* New steering vectors of the handle's shape / a new loading (validated as at create), used from
 * the next call on: the result then equals a fresh handle created with them, bit for bit.  May
 * block until the handle's earlier calls have finished; never changes what an already enqueued
 * call computes. */
int sfe_dsp_mvdr_set_steering(sfe_mvdr_t h, const float *steering);
int sfe_dsp_mvdr_set_loading(sfe_mvdr_t h, float load_rel, float load_abs);
/* n_rows rows of every band, layouts as above.  *n_out = n_rows.  n_rows = 0 is a no-op;
 * n_rows >= 2^31 / (2S)^2 is SFE_EINVAL.  out_stride < M*4BS, power_stride < M*B (with d_power)
 * and status_stride < M (with d_status) are SFE_ERANGE; in_stride < n_rows*(2S)^2, a null d_gram
 * or d_real_matrix, misaligned buffers and an output byte range that overlaps the input's are
 * SFE_EINVAL; nothing is launched on a refusal.  Asynchronous on `stream`; allocates nothing,
 * does not synchronise the host, carries no state (there is no reset).  A call on a stream under
 * graph capture is SFE_ESTATE, nothing enqueued: sfe_dsp_mvdr_set_steering may replace the tables
 * a captured call would have pinned. */
/* A stride that takes a buffer's byte range to 2^62 is SFE_EINVAL too; nothing is launched. */
int sfe_dsp_mvdr_process_stream(sfe_mvdr_t h, const void *d_gram, size_t n_rows, size_t in_stride,
                                void *d_real_matrix, size_t out_stride, void *d_power,
                                size_t power_stride, void *d_status, size_t status_stride,
                                size_t *n_out, sfe_stream_t stream);
/* Hands a device matrix to a live beamformer: enqueues on `stream` a small kernel that rewrites
 * the handle's weight table from d_real_matrix, [M][2B][2S] float32 of the handle's own shape
 * (one row block of sfe_dsp_mvdr_process_stream's output, or sfe_dsp_beam_plan's real_matrix).
 * Beamformer calls enqueued later on the same stream use it, calls enqueued before it keep the
 * old weights; calls on other streams are the caller's to order.  The host touches nothing and
 * does not wait.  Values are not checked: a non-finite entry poisons as the beamformer documents.
 * A handle that is not a live beamformer, a null or misaligned matrix: SFE_EINVAL; a stream under
 * graph capture: SFE_ESTATE; nothing enqueued either way. */
int sfe_dsp_mvdr_load_beam(sfe_beam_t beam, const float *d_real_matrix, sfe_stream_t stream);
int sfe_dsp_mvdr_destroy(sfe_mvdr_t h);

/* --------------------------------- symmetric eigen-decomposition / MUSIC direction finder
 * What stands at the head of the array chain, on the device: per (output row j of sfe_dsp_cov_*,
 * band k) the eigenvalues of the Gram matrix (how many signals there are, and how strong), the
 * MUSIC null spectrum of B scan steering vectors (where they are: the directions the weight
 * solver above is then given), and the E leading eigenvectors as a real matrix the beamformer
 * multiplies by (a signal-subspace beamformer).
 * The law, on real matrices (n = 2S; G the n x n float32 Gram matrix; float32 on the device):
 *   1. Read.  Only G[i][j] with i <= j is read; the lower triangle is taken as its mirror.
 *   2. Structure.  widely_linear = 1: G^ = G.  widely_linear = 0 (the covariance C alone, the
 *      pseudo-covariance ignored):
 *          G^[2s][2t]   =  G^[2s+1][2t+1] = (G[2s][2t] + G[2s+1][2t+1]) / 2
 *          G^[2s+1][2t] = -G^[2s][2t+1]   = (G[2s+1][2t] - G[2s][2t+1]) / 2
 *      (half the realification of C: its eigenvalues are those of C, halved, each twice).  There
 *      is no diagonal loading.
 *   3. Decompose.  G^ = V diag(lambda) V^T by the two-sided cyclic Jacobi method: right for every
 *      finite symmetric G^, singular (fewer snapshots than n) and indefinite ones included.  G^ is
 *      first scaled by the power of two that brings its largest |entry| into [1, 2) -- exactly,
 *      subnormal entries included; the eigenvalues are scaled back (exactly, unless the result
 *      is subnormal: then rounded once).
 *      Widely linear: the method runs on the n x n matrix A = G^.  A sweep is n - 1 steps of
 *      n / 2 disjoint pairs in round-robin order, a function of n alone: step r pairs n - 1 with
 *      r, and (r + a) mod (n - 1) with (r - a) mod (n - 1) for a = 1 .. n / 2 - 1.  A pair (p, q),
 *      p < q, whose coupling A[p][q] is exactly zero is NOT rotated (a diagonal G^ comes out
 *      exact); any other is rotated by theta = (A[q][q] - A[p][p]) / (2 A[p][q]),
 *      t = sign(theta) / (|theta| + sqrt(theta^2 + 1)), c = 1 / sqrt(t^2 + 1), s = t c: A[p][p]
 *      -= t A[p][q], A[q][q] += t A[p][q], the coupling set to exactly zero, every other entry of
 *      rows and columns p, q and the accumulated V (which starts as I) rotated by (c, s).
 *      Linear: G^ is the realification of the S x S Hermitian Z, Z[s][t] = G^[2s][2t] +
 *      j G^[2s+1][2t], and the method runs on Z with the same order over S indices (an odd S gets
 *      one more, whose row and column are zero: never rotated, never reported): the coupling
 *      Z[p][q] = m w, |w| = 1, is annihilated by the unitary diag(1, conj w) times the rotation
 *      above for the coupling m.  A complex eigenvector w stands for the two real ones u(w) and
 *      u(jw) of G^, and its eigenvalue is written twice.  This is what makes the eigenvectors of a
 *      repeated or clustered eigenvalue come out as exact (u(w), u(jw)) pairs; a real method on
 *      G^ cannot promise that.
 *      Either way the method stops after the first sweep in which no coupling it met exceeded
 *      2^-27 in magnitude (after the scaling; float64 plan: 2^-56) -- that sweep's rotations are
 *      still applied; a sweep that rotates nothing is one such -- and after 30 sweeps at the
 *      latest.  Eigenvalues in descending algebraic order, equal ones in
 *      the order of their position on the diagonal.  Each eigenvector is divided by its computed
 *      norm and signed so that its largest-magnitude real component (the first of equals) is
 *      positive.
 *   4. Null spectrum.  The signal subspace is spanned by the first D = signal_dim eigenvectors
 *      (REAL dimensions: a circular source takes 2, a rectilinear source takes 1 in the
 *      widely-linear mode; D is even in the linear mode); N = V[:, D:].  Per beam b, a its steering
 *      vector, u(a)[2s] = Re a_s, u(a)[2s+1] = Im a_s, A2 = [u(a), u(ja)]:
 *      Q = (N^T A2)^T (N^T A2), 2 x 2, Q[0][1] used for both off-diagonal entries -- sums of
 *      squares and products over the noise eigenvectors, so nothing cancels (linear mode: the
 *      pair u(w), u(jw) contributes |w^H a|^2 to both diagonal entries and nothing beside them,
 *      and that is how Q = q I is formed) -- and
 *          null_b = max(lambda_min(Q), 0) / |a|^2,   in [0, 1] up to rounding,
 *      lambda_min by the closed form (Q00 + Q11) / 2 - sqrt(((Q00 - Q11) / 2)^2 + Q01^2).
 *      The MUSIC pseudo-spectrum is 1 / null_b: left to the caller, because null_b may be 0.
 *   5. Eigen-beams.  The E = n_vec leading vectors as one [2E][2S] block per band, the layout of
 *      sfe_dsp_beam_plan's real_matrix for E beams (sfe_dsp_mvdr_load_beam takes it as it is).
 *      Widely linear: rows 2e, 2e+1 are eigenvectors 2e, 2e+1.  Linear: row 2e is eigenvector 2e
 *      (u(w) of the e-th complex eigenvector) and row 2e+1 its exact rotation u(jw),
 *      R[2e+1][2s] = -R[2e][2s+1], R[2e+1][2s+1] = R[2e][2s]: the matrix of the complex W = w^H
 *      with V absent.
 *   6. Failure never writes a NaN weight.  A problem fails if an entry of G^ (linear mode: or the
 *      sum or difference of step 2 before its halving) is not finite in float32, or at the sweep
 *      limit: status 1, its eigenvalues and null spectrum quiet NaN, its eigen-beams the
 *      selection matrix of streams 0 .. E-1 (R[r][r] = 1, zero elsewhere).  Status 0 otherwise.
 * Layouts.  Input as sfe_dsp_mvdr_*: row j of band k at d_gram + k*in_stride + j*(2S)^2 floats.
 * Outputs: values [n_rows][M][2S] at d_values + j*values_stride + k*2S; null [n_rows][M][B] at
 * d_null + j*null_stride + k*B + b; vectors [n_rows][M][2E][2S] at d_vectors + j*vectors_stride +
 * k*4ES; status (int32) at d_status + j*status_stride + k.  null, vectors and status may each be
 * NULL.  All 4-byte aligned.
 * Shapes: 1 <= S <= 64, 0 <= B <= 64, 0 <= E <= S, 1 <= M <= 1024, M*max(B,E,1)*S <= 2^20,
 * 0 <= D < 2S (even in the linear mode), every steering value finite and every steering vector
 * non-zero (steering may be NULL with B = 0), widely_linear 0 or 1; anything else is SFE_EINVAL
 * with a message that starts with "eig: ".
 * Contracts about bits:
 *   1. the same calls give the same bits on every run;
 *   2. a problem's output depends on its own G, its band's steering and the parameters only:
 *      never on M, n_rows, j, addresses or strides; band k of an M-band handle gives the bits of
 *      a one-band handle holding band k's steering;
 *   3. null_b depends on a_b only: a B-beam handle reproduces B one-beam handles;
 *   4. nothing of the strict lower triangle of G is read;
 *   5. in the linear mode the eigen-beams have the exact W-only structure of step 5;
 *   6. a diagonal G^ of distinct powers of two, negative ones included, gives its exact sorted
 *      eigenvalues, exact unit vectors, and exact 0 / 1 null values on selection steering vectors;
 *   7. a failed problem gets exactly the fallback bits, its neighbours are untouched;
 *   8. nothing outside the rows written is touched.
 * Not promised: the bits of the host plan or of LAPACK, equal bits between different S, the basis
 * inside a degenerate eigenvalue's plane (in the linear mode: the phase of a complex
 * eigenvector).
 * Computed by csrc/eig.hip: one workgroup per problem, the matrix and V^T in LDS (up to 131 KB
 * widely linear, 67 KB linear, taken per launch), two barriers per step. */
typedef void *sfe_eig_t; /* opaque: M bands of B scan vectors over S streams, a mode, D and E */
/* Host-only (no GPU): validates the arguments as above.  If gram != NULL it decomposes ONE row --
 * M matrices [M][2S][2S], band-major -- by the law in float64 and rounds once to float32 into
 * values [M][2S] (required then), null_spectrum [M][B], vectors [M][2E][2S] and status [M], each
 * of which may be NULL: the CPU fallback, and the reference of the device's values (not of its
 * bits).
 *   steering  [n_bands][n_beams][n_in] (re, im) float32 pairs */
int sfe_dsp_eig_plan(int n_in, int n_beams, int n_vec, int n_bands, const float *steering,
                     int widely_linear, int signal_dim, const float *gram, float *values,
                     float *null_spectrum, float *vectors, int *status);
/* The steering vectors are copied.  Arguments are checked before the device is touched:
 * SFE_EINVAL for a bad one on any machine, SFE_ENODEV without a GPU. */
int sfe_dsp_eig_create(const float *steering, int n_in, int n_beams, int n_vec, int n_bands,
                       int widely_linear, int signal_dim, int device, sfe_eig_t *out);
/* New scan vectors of the handle's shape / a new signal dimension (validated as at create), used
 * from the next call on: the result then equals a fresh handle created with them, bit for bit.
 * set_steering may block until the handle's earlier calls have finished; neither changes what an
 * already enqueued call computes. */
int sfe_dsp_eig_set_steering(sfe_eig_t h, const float *steering);
int sfe_dsp_eig_set_signal_dim(sfe_eig_t h, int signal_dim);
/* n_rows rows of every band, layouts as above.  *n_out = n_rows.  n_rows = 0 is a no-op;
 * n_rows >= 2^31 / (2S)^2 is SFE_EINVAL.  values_stride < M*2S, null_stride < M*B (with d_null),
 * vectors_stride < M*4ES (with d_vectors) and status_stride < M (with d_status) are SFE_ERANGE;
 * in_stride < n_rows*(2S)^2, a null d_gram or d_values, misaligned buffers and an output byte
 * range that overlaps the input's are SFE_EINVAL; nothing is launched on a refusal.  Asynchronous
 * on `stream`; allocates nothing, does not synchronise the host, carries no state (there is no
 * reset).  A call on a stream under graph capture is SFE_ESTATE, nothing enqueued:
 * sfe_dsp_eig_set_steering may replace the table a captured call would have pinned. */
/* A stride that takes a buffer's byte range to 2^62 is SFE_EINVAL too; nothing is launched. */
int sfe_dsp_eig_process_stream(sfe_eig_t h, const void *d_gram, size_t n_rows, size_t in_stride,
                               void *d_values, size_t values_stride, void *d_null,
                               size_t null_stride, void *d_vectors, size_t vectors_stride,
                               void *d_status, size_t status_stride, size_t *n_out,
                               sfe_stream_t stream);
int sfe_dsp_eig_destroy(sfe_eig_t h);

/* ------------------------------------------------- feed-forward burst demodulator
 * What follows the correlator: for each burst a window of one stream, whose start offset lies in
 * device memory where sfe_dsp_corr_* wrote it, becomes N symbol-rate samples that are timing-,
 * frequency-, phase- and amplitude-corrected, with a record of the estimates and a status.  Nothing
 * is carried from burst to burst; no host read or copy lies between the two blocks.
 * Shapes: sps (samples per symbol) in [4, 64]; n_sym = N in [2, 4096], the preamble included; the
 * preamble p[0..Lp), 2 <= Lp <= N, every value finite, E_p = sum |p|^2 (float64, rounded once) > 0;
 * lag = D in [1, Lp); timing_mode 0 (estimate) or 1 (tau = 0); min_gate finite; n_streams >= 1;
 * anything else is SFE_EINVAL with a message that starts with "burst: ".
 * Burst b of stream s starts at o = start_base + b*start_step + idx (signed 64-bit), idx the uint32
 * at d_idx + s*idx_stride + b (0 with d_idx NULL).  Behind a one-template correlator of block B and
 * template length L: d_idx = its d_peak_idx, start_step = B, start_base = -(L-1) + the index of the
 * correlator's block 0 within the input buffer, d_gate = its d_peak_val.  With x stream s, float32
 * except where float64 is named:
 *   0  gate, range   with d_gate, a burst whose gate value is not >= min_gate (a NaN is not) has
 *                    status 2; a burst whose reach [o - sps, o + (N+1) sps) is not inside [0, n_in)
 *                    has status 3.  Neither reads a sample.
 *   1  timing        c = sum_{i < N sps} |x[o+i]|^2 w[i mod sps], w[r] = exp(-j 2 pi r / sps) from a
 *                    table made in float64 and rounded once; tau = -sps arg(c) / (2 pi) samples, in
 *                    (-sps/2, sps/2] (Oerder-Meyr).  timing_mode 1: tau = 0.
 *   2  interpolate   m = floor(tau), mu = tau - m, cubic Lagrange once per burst:
 *                    L-1 = -mu(mu-1)(mu-2)/6, L0 = (mu+1)(mu-1)(mu-2)/2, L1 = -(mu+1)mu(mu-2)/2,
 *                    L2 = (mu+1)mu(mu-1)/6;  y[k] = sum_{q=-1..2} L_q x[o + k sps + m + q], k < N,
 *                    an fmaf chain from +0 in that order of q, per component.
 *   3  carrier       z[k] = y[k] conj(p[k]), k < Lp;  R = sum_{k < Lp-D} z[k+D] conj(z[k]);
 *                    f = arg(R) / (2 pi D) turns per symbol, |f| <= 1/(2D);
 *                    S = sum_{k < Lp} z[k] exp(-j 2 pi f k);  theta = arg(S) / (2 pi) turns;
 *                    a = |S| / E_p.
 *   4  phase         wherever exp(-j 2 pi (theta + f k)) is needed (in S with theta = 0, and in 5)
 *                    the turn count is formed in float64 from the float32 f and theta, reduced to
 *                    [-1/2, 1/2] by subtracting rint, and only then taken to float32.
 *   5  output        y^[k] = y[k] exp(-j 2 pi (theta + f k)) / a, k < N, cf32 at
 *                    d_out + (s*n_bursts + b)*out_stride + k.  The record, 8 float32 at
 *                    d_rec + (s*n_bursts + b)*8: tau, f, theta, a, q = |S|^2 / (E_p sum_{k<Lp} |y[k]|^2),
 *                    evm = sum_{k<Lp} |y^[k] - p[k]|^2 / E_p, +0, +0.  The status, int32 at
 *                    d_status + s*status_stride + b: 0.
 *   6  failure       a c, R or S that is zero or not finite, an a that is not > 0 and finite, or a
 *                    non-finite sample in the reach: status 1.  A burst of status 1, 2 or 3 gets N
 *                    symbols of +0 and a record of quiet NaN whose words 6 and 7 are still +0.
 * Promised about bits: the same calls give the same bits on every run (no floating-point atomics); a
 * burst's output depends on its reach, the preamble and the parameters only -- never on b, s,
 * n_bursts, addresses, strides or whether windows overlap, which they may; u8 input gives the bits
 * of the cf32 path on the converted samples; with timing_mode 1, p all ones and x = 1+0j constant,
 * f = theta = +0, a = q = 1, evm = 0 and y^ is exactly 1+0j; nothing outside the slots named is
 * written.  Not promised: the order of the three sums (fixed per (sps, N, Lp, D)), equal bits
 * between shapes, the bits of the host plan. */
typedef void *sfe_burst_t;  /* opaque: one demodulator over n_streams streams */
/* Host-only (no GPU): validates what create validates (one stream).  With x != NULL -- n_in cf32
 * samples of ONE stream -- it runs n_bursts bursts by the law in float64 (idx [n_bursts] and gate
 * [n_bursts] host arrays, either may be NULL), each estimate rounded to float32 where the law hands
 * it on, and rounds once to float32 into symbols [n_bursts][N] cf32 (required then), record
 * [n_bursts][8] and status [n_bursts] (each may be NULL): the CPU fallback, and the reference of the
 * device's values (not of its bits).  With given != NULL, [n_bursts][8] float32, steps 1 and 3 are
 * skipped and tau, f, theta, a are words 0..3 of given; a burst whose given words are not usable
 * (not finite, |tau| > sps/2, a not > 0) has status 1.  n_in or n_bursts >= 2^31, or a
 * start_base + b*start_step beyond +-(2^63 - 2^33) for some burst, is SFE_EINVAL. */
int sfe_dsp_burst_plan(const float *preamble, int n_pre, int sps, int n_sym, int lag,
                       int timing_mode, float min_gate, const float *x, size_t n_in,
                       const uint32_t *idx, const float *gate, size_t n_bursts, int64_t start_base,
                       int64_t start_step, const float *given, float *symbols, float *record,
                       int *status);
/*   preamble  [n_pre] complex float32 as (re, im) pairs (copied)
 * Arguments are checked before the device is touched: SFE_EINVAL for a bad one on any machine,
 * SFE_ENODEV without a GPU. */
int sfe_dsp_burst_create(const float *preamble, int n_pre, int sps, int n_sym, int lag,
                         int timing_mode, float min_gate, int n_streams, int device,
                         sfe_burst_t *out);
/* SFE_FMT_F32 (cf32 input, 8-byte aligned) or SFE_FMT_U8 ((I,Q) byte pairs, 2-byte aligned,
 * converted (b-128)*(1/127) on load exactly as sfe_dsp_rx_u8_to_f32); any other format is
 * SFE_EINVAL. */
int sfe_dsp_burst_set_input_format(sfe_burst_t h, int fmt);
/* A new min_gate (finite), used from the next call on; an enqueued call keeps the one it took. */
int sfe_dsp_burst_set_gate(sfe_burst_t h, float min_gate);
/* n_bursts bursts of every stream: stream s at d_in + s*in_stride (samples of the input format),
 * n_in samples long; the other layouts as above.  d_idx, d_gate, d_rec and d_status may each be
 * NULL.  *n_out = n_bursts; n_bursts = 0 is a no-op.  out_stride < N, or status_stride < n_bursts
 * with d_status, is SFE_ERANGE; a null d_in or d_out, misaligned buffers (cf32 8 bytes, u8 pairs 2,
 * the rest 4), in_stride < n_in with more than one stream, n_in >= 2^31, n_streams*n_bursts >= 2^31,
 * a start_base + b*start_step beyond +-(2^63 - 2^33) for some burst, a stride that takes a
 * buffer's byte range to 2^62
 * and any output byte range that overlaps the input's, the index table's, the gate table's or
 * another output's are SFE_EINVAL; nothing is launched on a refusal.  Asynchronous on `stream`;
 * allocates nothing, does not synchronise the host, carries no state (there is no reset).  A call on
 * a stream under graph capture is SFE_ESTATE, nothing enqueued: sfe_dsp_burst_set_gate may change
 * what a captured call would have pinned. */
int sfe_dsp_burst_process_stream(sfe_burst_t h, const void *d_in, size_t n_in, size_t in_stride,
                                 const void *d_idx, size_t idx_stride, const void *d_gate,
                                 size_t gate_stride, size_t n_bursts, int64_t start_base,
                                 int64_t start_step, void *d_out, size_t out_stride, void *d_rec,
                                 void *d_status, size_t status_stride, size_t *n_out,
                                 sfe_stream_t stream);
int sfe_dsp_burst_destroy(sfe_burst_t h);

/* ------------------------------------------------- soft-decision Viterbi decoder
 * What follows the burst demodulator on a coded link: per burst, n_soft soft values -- float32, or
 * the components of the symbols sfe_dsp_burst_* wrote, where they lie on the device -- become the
 * ceil(n_info / 8) bytes of the payload, a record and a status.  Bursts are independent; nothing is
 * carried.  All arithmetic is float32, and every operation is ONE IEEE addition or comparison: no
 * product, no fused operation.
 * Code: constraint length K in [3, 9]; n_gen = n generators, n in {2, 3, 4}, 0 < g_j < 2^K;
 * S = 2^(K-1) states; a state is the K-1 latest input bits, newest in bit 0.  Input bit u from state
 * s: reg = (s << 1 | u) mod 2^K, coded bit c_j = parity(reg & g_j) for j = 0 .. n-1 in that order,
 * next state reg mod S.  The encoder starts in state 0.  terminated = 1: K-1 zero bits follow the
 * n_info payload bits, T = n_info + K-1 steps, the decoder ends in state 0; terminated = 0:
 * T = n_info, the decoder ends in the state of the largest metric, the lowest index among equals.
 * n_info in [1, 8192].
 * Puncturing: keep[P][n] bytes of 0 / 1, period P in [1, 32] steps, at least one position kept;
 * keep = NULL: every position is kept (P is then ignored).  Position (t, j) is transmitted iff
 * keep[t mod P][j]; the kept positions, numbered in the order of (t, j), are the indices of the
 * burst's soft values: n_soft of them over the T steps (a pattern that keeps none of them is
 * refused).  A punctured position has the soft value +0 and consumes no input.
 * Soft input: r > 0 favours coded bit 0.  SFE_VIT_IN_SOFT: n_soft float32 per burst at
 * d_in + b*in_stride (skip must be 0).  SFE_VIT_IN_BPSK: d_in is rows of cf32 as sfe_dsp_burst_*
 * writes them, soft value i is Re of symbol skip + i.  SFE_VIT_IN_QPSK: soft value 2i is Re and
 * 2i+1 is Im of symbol skip + i.  skip in [0, 2^24] is the preamble's length; in_stride counts
 * elements of the mode's type.  Behind a burst demodulator: its d_out, its out_stride, skip = Lp and
 * its d_status as d_status_in are the whole glue.
 * Metrics: pm[0] = +0, pm[s] = -inf elsewhere.  Step t, state s', u = s' & 1: the predecessors are
 * p0 = s' >> 1 and p1 = p0 | S/2; the branch value bm(p) = ((+-r_0) + (+-r_1)) + ..., left to right
 * over the step's n positions, minus (the sign bit flipped) where the branch's c_j is 1;
 * cand0 = pm[p0] + bm(p0), cand1 = pm[p1] + bm(p1); decision d = (cand1 > cand0);
 * pm'[s'] = d ? cand1 : cand0 -- equal candidates take p0.  No normalisation, no renormalising
 * subtraction: T n max|r| stays far inside float32's range.
 * Traceback: from the end state, for t = T-1 .. 0: bit_t = s & 1, s = (s >> 1) | (d_t[s] << (K-2)).
 * Output per burst: bits 0 .. n_info-1 packed MSB-first into ceil(n_info / 8) bytes at
 * d_bits + b*out_stride (bytes), pad bits 0; a record of two 32-bit words at d_rec + 2b -- the end
 * state's metric as float32, and a uint32 count of the kept positions whose re-encoded bit disagrees
 * with the sign of r (r = +-0 agrees with either bit); an int32 status at d_status + b:
 *   0  decoded
 *   1  a non-finite soft value among the burst's n_soft: the bytes are 0, the record (quiet NaN
 *      0x7fc00000, 0)
 *   2  d_status_in is given and its word for this burst is not 0 (the table sfe_dsp_burst_* wrote):
 *      no input is read; bytes and record as for status 1
 * Promised about bits: the same call gives the same bits on every run; a burst's output depends on
 * its n_soft values and the code only -- never on b, n_bursts, addresses, strides or the input mode
 * (BPSK and QPSK input give the bits of SOFT input on the extracted components); the device's
 * bytes, metric word, count and status EQUAL sfe_dsp_vit_plan's, for every input whose partial sums
 * are zero or normal numbers; nothing outside the slots named is written.  Not promised: anything
 * when a partial sum is subnormal or leaves float32's range.
 * A bad argument is SFE_EINVAL on any machine, with a message that starts with "vit: ". */
#define SFE_VIT_IN_SOFT 0
#define SFE_VIT_IN_BPSK 1
#define SFE_VIT_IN_QPSK 2
typedef void *sfe_vit_t;  /* opaque: one decoder; it owns no device memory and nothing in it changes after create */
/* Host-only, the transmit half: bits[n_info] (one 0 / 1 byte per bit) -> the kept coded bits, one
 * 0 / 1 byte each, in coded[*n_coded], termination and puncturing applied.  *n_coded = n_soft is
 * reported with coded = NULL too. */
int sfe_dsp_vit_encode(int K, int n_gen, const uint32_t *gen, const uint8_t *keep, int P,
                       int terminated, const uint8_t *bits, size_t n_info, uint8_t *coded,
                       size_t *n_coded);
/* Host-only: the LDS one burst needs on the device whatever its soft values do -- survivors,
 * T * max(S, 64) / 8 bytes, plus the packed bits, ceil(n_info / 8) rounded up to 8 -- whether the
 * T n soft values are staged beside them (all three within 134 400 bytes), and how many bursts
 * share a workgroup (0: create refuses the shape, the first two exceed 134 400 bytes). */
int sfe_dsp_vit_footprint(int K, int n_gen, int terminated, int n_info, size_t *lds_bytes,
                          int *staged, int *bursts_per_group);
/* Host-only (no GPU): validates what create validates and reports n_soft.  With in != NULL -- host
 * memory laid out as d_in of process_stream, status_in [n_bursts] or NULL likewise -- it decodes
 * n_bursts bursts by the law above, exactly as stated, into bytes (required then; burst b at
 * bytes + b*out_stride), record [n_bursts][2] and status [n_bursts] (each may be NULL): the CPU
 * fallback, and the reference of the device's bits.  Short strides are SFE_ERANGE. */
int sfe_dsp_vit_plan(int K, int n_gen, const uint32_t *gen, const uint8_t *keep, int P,
                     int terminated, int n_info, int in_mode, int skip, const float *in,
                     size_t in_stride, const int *status_in, size_t n_bursts, uint8_t *bytes,
                     size_t out_stride, uint32_t *record, int *status, size_t *n_soft);
/* Arguments are checked before the device is touched: SFE_EINVAL for a bad one on any machine
 * (a burst whose survivors and bits exceed the launch's LDS among them: K = 9 beyond T = 4183),
 * SFE_ENODEV without a GPU.  gen and keep are copied. */
int sfe_dsp_vit_create(int K, int n_gen, const uint32_t *gen, const uint8_t *keep, int P,
                       int terminated, int n_info, int in_mode, int skip, int device,
                       sfe_vit_t *out);
/* n_bursts bursts; d_status_in, d_rec and d_status may each be NULL.  *n_out = n_bursts;
 * n_bursts = 0 is a no-op.  in_stride below the row a burst reads (n_soft floats; skip + n_soft or
 * skip + ceil(n_soft / 2) symbols) or out_stride < ceil(n_info / 8) is SFE_ERANGE; a null d_in or
 * d_bits, misaligned buffers (soft values, records, statuses 4 bytes, symbols 8), n_bursts >= 2^31,
 * a stride that takes a buffer's byte range to 2^62, and any output byte range that overlaps an
 * input's or another output's are SFE_EINVAL; nothing is launched on a refusal.  Asynchronous on
 * `stream`; one kernel launch and nothing else: allocates nothing, does not synchronise the host,
 * carries no state (there is no reset).  Everything a call uses travels with it by value and a
 * handle has no setter, so a call on a stream under graph capture IS supported: the captured node
 * replays the same decoder on the same buffers. */
int sfe_dsp_vit_process_stream(sfe_vit_t h, const void *d_in, size_t in_stride,
                               const void *d_status_in, size_t n_bursts, void *d_bits,
                               size_t out_stride, void *d_rec, void *d_status, size_t *n_out,
                               sfe_stream_t stream);
int sfe_dsp_vit_destroy(sfe_vit_t h);

/* ------------------------------------------------- burst modulator, bytes to waveform
 * The transmit mirror of the burst demodulator and the Viterbi decoder: per burst,
 * ceil(n_info / 8) packed payload bytes on the device become one pulse-shaped frame of complex
 * baseband samples at a stated place of an output stream, cf32 or the transmit wire format.
 * Bursts are independent; nothing is carried.  No NCO: frequency placement is sfe_dsp_combine_*'s.
 * Shape, fixed at create:
 * Code: K, n_gen, gen, keep, P, terminated, n_info exactly as sfe_dsp_vit_* defines and validates
 * them (the same checker).  n_gen = 0 means UNCODED: the coded bits are the payload bits; K, gen,
 * keep, P and terminated are ignored.  n_info in [1, 8192].  n_soft: the number of kept coded
 * positions (n_info when uncoded).
 * Mapping: order 2 or 4, the maps SFE_VIT_IN_BPSK / SFE_VIT_IN_QPSK undo.  BPSK: data symbol i =
 * (amp (1 - 2 c_i), +0).  Gray QPSK: data symbol i = (a4 (1 - 2 c_2i), a4 (1 - 2 c_2i+1)) with
 * a4 = float32(amp / sqrt 2), formed in float64 and rounded once; an odd n_soft is padded with a 0
 * bit.  n_data = n_soft or ceil(n_soft / 2).  amp is finite and > 0.
 * Preamble: p[0 .. Lp) cf32, 0 <= Lp <= 4096, every value finite; the transmitted preamble symbol
 * is amp p[k], one float32 product per component.  N = Lp + n_data symbols s[0 .. N), the preamble
 * first.
 * Pulse: h[0 .. n_taps) real float32, finite; sps in [1, 64]; 1 <= n_taps <= 64 sps;
 * Q = ceil(n_taps / sps) <= 64 taps per arm; h[i] = 0 for i >= n_taps.
 * Frame: F = (N + Q - 1) sps samples.
 * Output format: SFE_FMT_F32 or SFE_FMT_TX10, given at create; there is no setter.
 * Bits: payload bit t of burst b is bit 7 - (t mod 8) of byte floor(t / 8) at d_bytes + b*in_stride
 * (MSB-first, the layout sfe_dsp_vit_* writes); pad bits are ignored.  u_t = 0 for t < 0 and for
 * t >= n_info (the termination tail).  Coded bit (t, j) = parity(reg_t & g_j), bit i of reg_t being
 * u_(t-i), i < K, for t < T = n_info + (terminated ? K - 1 : 0).  The kept positions, numbered in
 * the order of (t, j), are coded bits 0 .. n_soft - 1: what sfe_dsp_vit_encode gives.
 * Waveform: frame sample i = k sps + r, 0 <= r < sps, 0 <= k < N + Q - 1:
 *   y[i] = sum over q = 0 .. Q-1 of h[q sps + r] s[k - q],
 * the terms with k - q outside [0, N) or q sps + r >= n_taps skipped; per component the sum is an
 * fmaf chain from +0 in increasing q.  A symmetric pulse of odd length therefore puts symbol k's
 * peak at frame sample k sps + (n_taps - 1) / 2.
 * Placement: a call defines EVERY sample of the output stream [0, n_out).  Burst b's frame occupies
 * [o_b, o_b + F), o_b = start_base + b*start_step; every sample in no frame is +0.  SFE_EINVAL,
 * nothing launched: start_base < 0; start_step < F with more than one burst (start_step is ignored
 * with one); o_(n_bursts-1) + F > n_out; n_out or n_bursts >= 2^31; an odd n_out under TX10.
 * n_bursts = 0 writes n_out zeros.
 * TX10: the bytes are exactly sfe_dsp_tx_f32_to_10bit's of the F32 output -- two complex samples
 * in 5 bytes, the groups aligned to the stream, not to frames: a frame may start in the middle of
 * a group.  (n_out / 2) * 5 bytes are written.
 * Promised about bits: the same call gives the same bits on every run; burst b's frame depends on
 * its bytes and the handle only -- never on b, n_bursts, addresses, strides or offsets; the
 * device's F32 words and TX10 bytes EQUAL sfe_dsp_mod_plan's, for every input whose partial sums
 * are zero or normal numbers (nothing is promised otherwise); nothing outside the n_out samples is
 * written.
 * A bad argument is SFE_EINVAL on any machine, with a message that starts with "mod: ". */
typedef void *sfe_mod_t;  /* opaque: one modulator; it owns its taps and its scaled preamble on the device and nothing in it changes after create */
/* Host-only: the samples of the stream one workgroup writes (a frame is cut into such tiles
 * wherever they fall, the Q - 1 symbols before a tile derived again) and the LDS it uses. */
int sfe_dsp_mod_footprint(int *tile_samples, size_t *lds_bytes);
/* Host-only (no GPU): validates what create validates and reports N, F and n_soft (each pointer
 * may be NULL); then the placement as process_stream does; then, with out != NULL, writes the
 * stream by the law above, exactly as stated -- n_out cf32 samples, or (n_out / 2) * 5 bytes under
 * SFE_FMT_TX10 -- from bytes (host memory laid out as d_bytes; required with n_bursts > 0): the
 * reference of the device's bits.  in_stride < ceil(n_info / 8) is SFE_ERANGE. */
int sfe_dsp_mod_plan(int K, int n_gen, const uint32_t *gen, const uint8_t *keep, int P,
                     int terminated, int n_info, int order, const float *preamble, int n_pre,
                     int sps, const float *taps, int n_taps, float amp, int out_fmt,
                     const uint8_t *bytes, size_t in_stride, size_t n_bursts, int64_t start_base,
                     int64_t start_step, size_t n_out, void *out, int *n_sym, int *frame_len,
                     size_t *n_soft);
/* Arguments are checked before the device is touched: SFE_EINVAL for a bad one on any machine,
 * SFE_ENODEV without a GPU.  gen, keep, preamble and taps are copied. */
int sfe_dsp_mod_create(int K, int n_gen, const uint32_t *gen, const uint8_t *keep, int P,
                       int terminated, int n_info, int order, const float *preamble, int n_pre,
                       int sps, const float *taps, int n_taps, float amp, int out_fmt, int device,
                       sfe_mod_t *out);
/* One stream of n_out samples holding n_bursts frames.  *n_written = n_out.  The placement
 * refusals above; in_stride < ceil(n_info / 8) is SFE_ERANGE; a null d_out, a null d_bytes with
 * bursts, a cf32 d_out that is not 8-byte aligned (TX10 output and the payload bytes need no
 * alignment), an in_stride that takes the payloads' byte range to 2^62 and an output byte range
 * that overlaps the payloads' are SFE_EINVAL; nothing is launched on a refusal.  n_out = 0 is a
 * no-op.  Asynchronous on `stream`; one kernel launch and nothing else: allocates nothing, does
 * not synchronise the host, carries no state (there is no reset).  A handle has no setter, so a
 * call on a stream under graph capture IS supported.  Behind a decoder: its d_bits and out_stride
 * are the whole glue (a regenerative relay). */
int sfe_dsp_mod_process_stream(sfe_mod_t h, const void *d_bytes, size_t in_stride, size_t n_bursts,
                               int64_t start_base, int64_t start_step, void *d_out, size_t n_out,
                               size_t *n_written, sfe_stream_t stream);
int sfe_dsp_mod_destroy(sfe_mod_t h);

/* ------------------------------------------------- streaming FM, phase and envelope detector
 * The stage between a tuned complex stream and a real signal: one real float32 output per complex
 * input sample of every stream, by one of three laws fixed at create.  With n the absolute sample
 * index since create / reset and x[-1] = 0 + 0j:
 *     SFE_POLAR_FM   y[n] = gain at2(im, re) of x[n] conj(x[n-1])     the quadrature discriminator
 *     SFE_POLAR_PM   y[n] = gain at2(x.i, x.r)
 *     SFE_POLAR_AM   y[n] = gain sqrtf(fmaf(x.r, x.r, x.i x.i))
 * so FM's first output on a fresh handle is +0.  Behind sfe_dsp_ddc_* (K tunings in one pass) and in
 * front of a real decimator and sfe_dsp_iir_* (de-emphasis, DC blocker) this is K FM, FSK or AM
 * receivers that never leave the device.
 * The law is csrc/polar_law.h, one header the kernel and the host plan both compile; every multiply
 * that feeds an add is an explicit fmaf and everything else is one IEEE float32 operation:
 *     FM:  re = fmaf(x.r, p.r, x.i p.i);   im = fmaf(x.i, p.r, -(x.r p.i));        p = x[n-1]
 *     at2(y, x):
 *       ax = |x|; ay = |y|; mx = max(ax, ay); mn = min(ax, ay);
 *       z = (mx == 0) ? 0 : mn / mx                       one correctly rounded division
 *       s = z z;  q = C8;  q = fmaf(q, s, C7); ... q = fmaf(q, s, C0);  r = q z
 *       if (ay > ax) r = PI_2 - r;   if (x < 0) r = PI - r;   if (y < 0) r = -r     (-0 is not below 0)
 * with PI_2 = 0x1.921fb6p+0f, PI = 0x1.921fb6p+1f and C0 .. C8 the literals of the header (a
 * weighted least-squares fit of atan(z)/z in z^2).  at2 is within 2 ulp(pi) = 4.77e-7 rad of atan2,
 * FM within 3 ulp(pi) = 7.15e-7 rad of the angle of the exact product, AM within 1.3e-7 relative
 * (DESIGN.md 4.19 has the measured figures).  at2(0, 0) = +0, at2(0, -1) = PI, at2(-0, -1) = PI.
 * Input: cf32, or SFE_FMT_U8 (I,Q) byte pairs converted (b-128)*(1/127) exactly as
 * sfe_dsp_rx_u8_to_f32 converts them; the law then runs on the converted floats.
 * Contracts about bits, for finite input:
 *   1. the device's output equals sfe_dsp_polar_plan's bit for bit;
 *   2. cutting the stream into calls of ANY sizes >= 1 gives the one-call output bit for bit, and so
 *      does moving a buffer to any element-aligned address or changing the strides: there is NO
 *      GRANULE;
 *   3. u8 input gives the bits of the cf32 path on the converted samples, and the format may change
 *      between calls (the carried sample is kept as float32);
 *   4. stream s of an n-stream handle gives the bits of a one-stream handle fed that stream;
 *   5. reset makes a fresh handle.
 * A non-finite sample makes at most the outputs that read it non-finite (two in FM, one otherwise);
 * nothing persists. */
#define SFE_POLAR_FM 0
#define SFE_POLAR_PM 1
#define SFE_POLAR_AM 2
typedef void *sfe_polar_t; /* opaque: one detector over n_streams streams */
/* Host-only (no GPU): the law on n_in samples of one stream in host memory (fmt: SFE_FMT_F32, n_in
 * (re, im) float32 pairs; SFE_FMT_U8, n_in (I,Q) byte pairs; any alignment), written to out[0 .. n_in).
 * prev is the carried sample, in and out: (re, im) of x[-1] on entry (0, 0 for a fresh stream),
 * the last sample as float32 on return (unchanged by n_in = 0); NULL stands for a fresh stream and
 * returns nothing.  Carried in every mode, read in FM only.  A mode or format other than the above,
 * a non-finite gain and a null buffer with n_in > 0 are SFE_EINVAL with a message that starts with
 * "polar: ". */
int sfe_dsp_polar_plan(int mode, float gain, int fmt, const void *in, size_t n_in, float prev[2],
                       float *out);
/*   n_streams  independent streams, each with its own carried sample (1 .. 32767).
 * mode, gain and n_streams are checked before the device ("polar: ..."): SFE_EINVAL for those on
 * any machine, SFE_ENODEV without a GPU. */
int sfe_dsp_polar_create(int mode, float gain, int n_streams, int device, sfe_polar_t *out);
/* SFE_FMT_F32 (cf32 input, 8-byte aligned) or SFE_FMT_U8 ((I,Q) byte pairs, 2-byte aligned); any
 * other format is SFE_EINVAL ("polar: ...").  A captured call keeps the format it was captured with. */
int sfe_dsp_polar_set_input_format(sfe_polar_t h, int fmt);
/* n_in samples of every stream: stream s at d_in + s*in_stride (samples of the input format) goes
 * to d_out + s*out_stride (float32, 4-byte aligned).  *n_out = n_in.  Any n_in >= 1 below 2^31;
 * n_in = 0 is a no-op.  out_stride < n_in is SFE_ERANGE; null or misaligned buffers, in_stride <
 * n_in with more than one stream, overlapping input and output byte ranges and n_in >= 2^31 are
 * SFE_EINVAL, each with a message that starts with "polar_process_stream: "; nothing is launched
 * on a refusal.  Asynchronous on `stream`; one kernel launch: allocates nothing, does not
 * synchronise the host and keeps no host counter, so a call on a stream under graph capture IS
 * supported: the carried sample is then copied back behind the launch instead of changing
 * buffers, so that every replay is the next call of the stream, and eager calls and replays may
 * interleave on one handle. */
int sfe_dsp_polar_process_stream(sfe_polar_t h, const void *d_in, size_t n_in, size_t in_stride,
                                 float *d_out, size_t out_stride, size_t *n_out, sfe_stream_t stream);
/* Zero the carried samples (a fresh handle). */
int sfe_dsp_polar_reset(sfe_polar_t h);
int sfe_dsp_polar_destroy(sfe_polar_t h);

/* ------------------------------------------------- spectrum occupancy detector over psd rows
 * From a row of N float32 spectrum bins to a decision, on the device: a robust noise floor (an exact
 * order statistic), a threshold, a morphological closing, and one compact record per emission --
 * where it is, how wide, its peak, its power and its first moment -- beside an optional per-bin
 * mask.  sfe_dsp_psd_* leaves its rows exactly where this block reads them, so psd -> occ runs
 * without the host, and a row of 16 KB goes down as 16 + 32 E bytes.  Stateless per row: no reset,
 * no host counter, nothing carried.
 * The law is csrc/occ_law.h, one header the kernel and the host plan both compile.  A row is
 * x[0..N); the parameters, fixed at create, are
 *     n_bins = N   8 <= N <= 4096, any integer; even when shift is set
 *     rank         0 <= rank < N          factor     float32, finite, > 0
 *     min_level    float32, finite        gap        0 <= gap < N
 *     min_width    1 <= min_width <= N    max_emissions = E, 1 <= E <= 64        shift  0 or 1
 *  1. Scan order.  xs[p] = x[(p + N - o) mod N], o = N/2 with shift and 0 without.  With shift, p
 *     walks psd's bins from frequency -1/2 upwards, so an emission across DC is one run.  The signed
 *     bin of position p is j = p - o: with shift, frequency j/N cycles per sample (what ddc wants).
 *  2. Non-finite rows.  If any value of the row is a NaN or an infinity: status bit 0 is set,
 *     count = 0, floor and thr are the word 0x7fc00000, all E records and the mask row are zero
 *     bytes, and nothing else is computed.
 *  3. Floor.  floor is the value of rank `rank` (0 = the smallest) of the row, in the total order of
 *     the keys  bits ^ (sign ? 0xffffffff : 0x80000000)  -- so -0 sorts below +0.  An exact
 *     selection: floor's bit pattern is that of an element of the row.
 *  4. Threshold and occupancy.  thr = fmaxf(factor * floor, min_level): one float32 multiply, and the
 *     greater of the two in the order of the keys (so of -0 and +0 it is +0: IEEE 754-2019's
 *     maximum).  occ[p] = xs[p] > thr, the float32 comparison.
 *  5. Closing.  c[p] is true when occ[p] is, or when there are occupied positions a < p < b, the
 *     nearest on each side, with b - a - 1 <= gap.  No wrap across the ends of the scan.
 *  6. Emissions.  The maximal runs [lo, hi] of c with hi - lo + 1 >= min_width, in ascending lo;
 *     count is how many there are.  count may exceed E: status bit 1 is set and the first E are
 *     recorded.
 *  7. Per emission.  peak_val is the maximum of xs over the run (the float32 comparison) and peak
 *     the smallest position that attains it.  sum and moment are folded over tiles of 16 aligned
 *     scan positions [16t, 16t + 16): a tile partial is the float32 left fold from +0, in ascending p
 *     over run and tile, of  acc + xs[p]  (sum)  and of  fmaf((float)(p - lo), xs[p], acc)  (moment);
 *     the emission's value is the float32 left fold from +0 of its tile partials in ascending t.
 *     The order is a function of positions only.  The caller's centroid is lo + moment / sum.
 *  8. Outputs for row slot q.  info[q]: floor, thr, count, status.  rec[q E + r], r < min(count, E):
 *     lo, hi, peak in signed bins, peak_val, sum, moment, two zero words; records r >= min(count, E)
 *     are zero bytes, so every byte of every output is written by every call.  The optional
 *     mask[q N + k] is 1 where bin k -- in the row's OWN numbering, whatever shift is -- lies in one
 *     of the `count` emissions (those beyond E included) and 0 elsewhere: used directly, a
 *     per-channel gate for a channelizer's output.
 * The only fused operation of the law is the fmaf of step 7; everything else is one IEEE float32
 * operation, a comparison, or integer work.
 * Contracts about bits:
 *   1. the device's bytes equal sfe_dsp_occ_plan's;
 *   2. a row's outputs depend on that row and the parameters only: never on its neighbours, its
 *      address, the strides, the call's size or the grid;
 *   3. with and without d_mask, info and rec are the same bytes. */
#define SFE_OCC_NONFINITE 1u /* status bit 0: the row held a NaN or an infinity */
#define SFE_OCC_TRUNCATED 2u /* status bit 1: count > max_emissions */
typedef struct {
    float floor, thr;
    uint32_t count, status;
} sfe_occ_info; /* 16 bytes */
typedef struct {
    int32_t lo, hi, peak; /* signed bins */
    float peak_val, sum, moment;
    uint32_t zero[2];
} sfe_occ_rec;            /* 32 bytes */
typedef void *sfe_occ_t; /* opaque: one detector */
/* Host-only (no GPU): the law on n_rows rows of n_bins float32 in host memory, row i at
 * rows + i*n_bins; info[i], rec[i*E ..], mask[i*n_bins ..].  Any output may be NULL.  Parameters
 * outside the ranges above are SFE_EINVAL with a message that starts with "occ: "; so is a null
 * `rows` with n_rows > 0.  With n_rows = 0 it validates the parameters. */
int sfe_dsp_occ_plan(int n_bins, int rank, float factor, float min_level, int gap, int min_width,
                     int max_emissions, int shift, const float *rows, size_t n_rows,
                     sfe_occ_info *info, sfe_occ_rec *rec, uint8_t *mask);
/* The parameters are checked before the device is touched ("occ: ..."): SFE_EINVAL for those on any
 * machine, SFE_ENODEV without a GPU. */
int sfe_dsp_occ_create(int n_bins, int rank, float factor, float min_level, int gap, int min_width,
                       int max_emissions, int shift, int device, sfe_occ_t *out);
/* n_rows rows of each of n_streams streams: row j of stream s is read at d_in + s*in_stride + j*N
 * floats -- where sfe_dsp_psd_process_stream leaves its rows -- and goes to slot q = s*out_stride + j
 * of every output: d_info[q], d_rec[q*E ..], d_mask[q*N ..] (d_mask may be NULL).
 * *n_done = n_streams * n_rows.  n_rows = 0 or n_streams = 0 is a no-op.  out_stride < n_rows is
 * SFE_ERANGE; null or misaligned buffers (float32, info and records 4 bytes), in_stride < n_rows*N
 * with more than one stream, an overlap between the input and any output or between two outputs,
 * and 2^31 or more rows are SFE_EINVAL, each with a message that starts with
 * "occ_process_stream: "; nothing is launched on a refusal.  Asynchronous on `stream`; one kernel
 * launch and nothing else: allocates nothing, does not synchronise the host, keeps no counter, so a
 * call on a stream under graph capture IS supported. */
int sfe_dsp_occ_process_stream(sfe_occ_t h, const float *d_in, size_t n_streams, size_t n_rows,
                               size_t in_stride, sfe_occ_info *d_info, sfe_occ_rec *d_rec,
                               uint8_t *d_mask, size_t out_stride, size_t *n_done,
                               sfe_stream_t stream);
int sfe_dsp_occ_destroy(sfe_occ_t h);

/* ------------------------------------------------- Reed-Solomon outer code, interleaved
 * What stands outside the convolutional code on a link: behind sfe_dsp_vit_* the decoder of an
 * interleaved Reed-Solomon code over GF(2^8), in front of sfe_dsp_mod_* its encoder, on the device.
 * A Viterbi decoder fails in bursts of wrong bytes; the interleave spreads a burst over I
 * codewords, the code corrects up to t bytes in each and says which codewords it could not
 * correct.  Frames are independent; nothing is carried.  Integer arithmetic only.
 * The law is csrc/reed_law.h, one header the kernels and the host plan both compile.
 * Field: GF(2^8) modulo prim, a 9-bit polynomial in [0x100, 0x1ff]; alpha is the element 0x02, and
 * prim is refused unless alpha has order 255 (0x11d and 0x187 pass; 0x11b does not: there x has
 * order 51).  The representation is the conventional one; there is no dual basis.
 * Code: n in [3, 255] (below 255: a shortened code), n_par in [2, 64] and n_par < n,
 * k = n - n_par, t = floor(n_par / 2); fcr in [0, 254]; step in [1, 254] with gcd(step, 255) = 1.
 * Byte j of a codeword is the coefficient of x^(n-1-j).  C is the set of words c of n bytes with
 * c(alpha^(step (fcr + i))) = 0 for i = 0 .. n_par-1.  Systematic: bytes 0 .. k-1 are the message,
 * the last n_par bytes are x^n_par m(x) mod g(x), g(x) the product of (x - alpha^(step (fcr + i))).
 * Interleave: depth I in [1, 16].  A payload is P = I k bytes, a frame Fb = I n bytes.  Message
 * byte j of codeword i is payload[j I + i]; codeword byte j of codeword i is frame[j I + i].  So
 * frame[0 .. P) is the payload as it lies, and the I n_par parity bytes follow.  A run of up to I t
 * consecutive wrong channel bytes is therefore always corrected: it puts at most t into any one
 * codeword.
 * Whitening: whiten is NULL or Fb bytes, copied at create.  The channel bytes are frame XOR whiten;
 * the decoder XORs first.  The sequence is the caller's: a PN generator stays outside the library.
 * Decode, per codeword: r is the de-whitened received word.  If some c in C has d(r, c) <= t it is
 * unique: the output message is c's and the codeword's count is d(r, c) (errors in parity bytes
 * count).  Otherwise the codeword is UNCORRECTABLE and its message bytes are r's as received.  For a
 * shortened code C holds only words of length n: an r whose nearest word of the full-length code
 * differs from it in a padded position is uncorrectable, not corrected.  There are no erasures:
 * sfe_dsp_vit_* delivers no per-byte reliability to feed them.  No CRC either: beyond t errors a
 * word may lie within t of ANOTHER codeword and decode to it (a miscorrection, by the same law).
 * Decode, per frame b: P bytes at d_out + b*out_stride; two uint32 words at d_rec + 2b -- the sum of
 * the counts of the corrected codewords, and a mask whose bit i is set iff codeword i is
 * uncorrectable; an int32 status at d_status + b:
 *   0  every codeword decoded
 *   1  at least one codeword is uncorrectable (the others are still corrected)
 *   2  d_status_in is given and its word for this frame is not 0: no input is read, the bytes are
 *      0, the record (0, 2^I - 1)
 * Encode, per frame: P payload bytes at d_payload + b*in_stride become Fb channel bytes at
 * d_frame + b*out_stride.
 * Promised about bytes: the same call gives the same bytes on every run; a frame's output depends
 * on its bytes and the handle only -- never on b, n_frames, addresses, alignment or strides; the
 * device's bytes, record and status EQUAL sfe_dsp_reed_plan's for every input, none excluded;
 * nothing outside the slots named is written, to the byte.  Payloads and frames need no alignment;
 * records and statuses 4 bytes.
 * Glue.  Behind sfe_dsp_vit_*: n_info = 8 Fb, so Fb <= 1024 (RS(255,223) at depth 4 is 1020 bytes);
 * the decoder's d_bits, out_stride and d_status are the whole glue.  In front of sfe_dsp_mod_*:
 * d_frame and out_stride are the whole glue.
 * A bad argument is SFE_EINVAL on any machine, with a message that starts with "reed: ". */
typedef void *sfe_reed_t; /* opaque: one code; it owns its tables (roots, generator, locators, whitening) on the device and nothing in it changes after create */
/* Host-only (no GPU): validates what create validates and reports P and Fb (each pointer may be
 * NULL).  With in != NULL -- host memory laid out as d_frame of process_stream (encode = 0) or as
 * d_payload of encode_stream (encode = 1) -- it runs n_frames frames by the law above, exactly as
 * stated, into out (frame b at out + b*out_stride), record [n_frames][2] and status [n_frames];
 * each of the three may be NULL.  status_in [n_frames] or NULL; with encode = 1 status_in, record
 * and status are ignored.  The reference of the device's bytes.  Short strides are SFE_ERANGE. */
int sfe_dsp_reed_plan(int prim, int fcr, int step, int n, int n_par, int depth,
                      const uint8_t *whiten, int encode, const uint8_t *in, size_t in_stride,
                      const int *status_in, size_t n_frames, uint8_t *out, size_t out_stride,
                      uint32_t *record, int *status, int *payload_bytes, int *frame_bytes);
/* Arguments are checked before the device is touched: SFE_EINVAL for a bad one on any machine,
 * SFE_ENODEV without a GPU.  whiten is copied. */
int sfe_dsp_reed_create(int prim, int fcr, int step, int n, int n_par, int depth,
                        const uint8_t *whiten, int device, sfe_reed_t *out);
/* n_frames frames each way.  d_status_in, d_rec and d_status may each be NULL.  *n_out = n_frames;
 * n_frames = 0 is a no-op.  A stride below the bytes a frame reads or writes (P, Fb) is SFE_ERANGE;
 * a null d_payload, d_frame or d_out, a misaligned record or status pointer, n_frames >= 2^31, a
 * stride that takes a buffer's byte range to 2^62, and any output byte range that overlaps an
 * input's or another output's are SFE_EINVAL, each with a message that starts with
 * "reed_encode_stream: " or "reed_process_stream: "; nothing is launched on a refusal.
 * Asynchronous on `stream`; one kernel launch and nothing else: allocates nothing, does not
 * synchronise the host, carries no state (there is no reset, and a handle has no setter), so a call
 * on a stream under graph capture IS supported.  Every loop of the kernels runs a number of times
 * fixed by (n, n_par): a corrupt frame cannot lengthen a launch. */
int sfe_dsp_reed_encode_stream(sfe_reed_t h, const void *d_payload, size_t in_stride,
                               size_t n_frames, void *d_frame, size_t out_stride, size_t *n_out,
                               sfe_stream_t stream);
int sfe_dsp_reed_process_stream(sfe_reed_t h, const void *d_frame, size_t in_stride,
                                const void *d_status_in, size_t n_frames, void *d_out,
                                size_t out_stride, void *d_rec, void *d_status, size_t *n_out,
                                sfe_stream_t stream);
int sfe_dsp_reed_destroy(sfe_reed_t h);

/* ------------------------------------------------- quasi-cyclic LDPC code, decoder and encoder
 * The inner code of a modern link beside the convolutional one: behind sfe_dsp_burst_* a layered
 * min-sum decoder, in front of sfe_dsp_mod_* (its uncoded mode, n_gen = 0) the encoder, on the
 * device.  Its parallelism is across the codeword, and its syndrome is its own frame check.
 * Codewords are independent; nothing is carried.  The decoder is integer arithmetic on a quantised
 * input.  The law's arithmetic is csrc/ldpc_law.h, one header the kernels and the host plan compile.
 * Code: a base matrix shift[mb][nb] of int16 (row-major) and a lifting size Z.  shift = -1 is an
 * empty cell, 0 <= shift < Z a circulant: row r Z + i of H has a one in column
 * c Z + (i + shift[r][c]) mod Z for every non-empty cell (r, c).  n = nb Z, m = mb Z, k = n - m.
 * Limits: Z in [1, 512] (Z = 1 makes any small H expressible); 1 <= mb <= 64; mb < nb <= 256;
 * n <= 8192; every block row has 2 to 32 cells; every block column at least one; cells Z <= 65 536.
 * Out of scope: more than one circulant per cell, punctured or shortened columns, erasure input.
 * Bits: a payload is k bits packed MSB-first into ceil(k / 8) bytes (the layout sfe_dsp_vit_*
 * writes), a codeword n bits packed MSB-first into ceil(n / 8) bytes (the layout sfe_dsp_mod_*
 * reads); pad bits are ignored on input and 0 on output.
 * Encode: the codeword c has c[0 .. k) = payload and H c = 0 over GF(2).  It exists and is unique
 * iff the last m columns of H are invertible: plan reports that as `encodable`; create accepts
 * either kind of matrix; encode_stream on a handle that is not encodable is SFE_ESTATE and launches
 * nothing.  The law names no algorithm for the parity bits.
 * Soft input: r > 0 favours bit 0.  The three modes SFE_VIT_IN_SOFT / _BPSK / _QPSK with `skip`,
 * exactly as sfe_dsp_vit_* defines them, on n soft values; in_stride counts elements of the mode's
 * type.  Behind a burst demodulator: its d_out, its out_stride, skip = Lp and its d_status as
 * d_status_in are the whole glue.
 * Quantisation: L_v = clamp(rintf(r_v * scale), -127, 127); the product is one float32 IEEE
 * multiply, rintf rounds ties to even, scale is finite and > 0 and fixed at create; a product that
 * overflows to +-inf clamps; a non-finite r_v is status 1.
 * Decoder: layered normalised and offset min-sum, all in integers.  State: APP[v], starting as L_v,
 * and one message R per edge, starting at 0.  Parameters fixed at create: a in [1, 16],
 * beta in [0, 127], max_iter in [1, 64].  One iteration visits the block rows l = 0 .. mb-1 in
 * order, and within a block row every i in [0, Z) (the Z rows of a layer touch disjoint variables:
 * their order cannot show).  For each row, with its cells j = 0 .. d-1 in increasing block column
 * and v_j the variable of cell j:
 *   Q_j = APP[v_j] - R_j;  neg_j = (Q_j < 0), zero counts as positive;  m1 = min_j |Q_j|;
 *   j* the lowest j attaining m1;  m2 = min over j != j* of |Q_j|;  M_j = (j == j*) ? m2 : m1;
 *   M'_j = min(max(((M_j a) >> 4) - beta, 0), 127);  S = XOR of all neg_j;
 *   R'_j = (S ^ neg_j) ? -M'_j : M'_j;  APP[v_j] = Q_j + R'_j;  R_j = R'_j.
 * Nothing else saturates: APP[v] always equals L_v plus the current messages of v's checks, so
 * |APP| <= 127 (1 + mb) <= 8255, which fits int16.  Decision: x_v = (APP[v] < 0).  The syndrome of x
 * is checked before the first iteration and after every complete one; decoding stops at the first
 * zero syndrome, or after max_iter iterations -- so `iterations` can be 0.
 * Output per codeword b: ceil(k / 8) bytes of x[0 .. k) at d_bits + b*out_stride; three uint32 at
 * d_rec + 3b -- iterations run, unsatisfied checks at the end (0 iff converged), the number of v
 * with L_v != 0 whose decision differs from the sign of L_v; an int32 status at d_status + b:
 *   0  converged
 *   1  a non-finite soft value: the bytes are 0, the record (0, 0, 0)
 *   2  d_status_in is given and its word for b is not 0: nothing is read, outputs as for status 1
 *   3  not converged after max_iter: the bytes are still the decisions
 * Promised: the same call gives the same bytes on every run; a codeword's output depends on its n
 * soft values and the handle only -- never on b, the count, addresses, strides or the input mode;
 * the device's bytes, record and status EQUAL sfe_dsp_ldpc_plan's for every input whose soft values
 * are finite, and a non-finite value is status 1 on both sides; nothing outside the slots named is
 * written, to the byte; a launch runs at most max_iter iterations, whatever the data.
 * A bad argument is SFE_EINVAL on any machine, with a message that starts with "ldpc: ". */
typedef void *sfe_ldpc_t; /* opaque: one code and its decoder's parameters; it owns its tables (cells, the parity part's inverse) on the device and nothing in it changes after create */
/* Host-only: the LDS a decoding workgroup uses and the codewords it holds (1, 2 or 4). */
int sfe_dsp_ldpc_footprint(int mb, int nb, int Z, const int16_t *shift, size_t *lds_bytes,
                           int *words_per_group);
/* Host-only (no GPU): validates what create validates and reports n, k and encodable (each pointer
 * may be NULL).  With in != NULL -- host memory laid out as d_in of process_stream (encode = 0) or
 * as d_payload of encode_stream (encode = 1) -- it runs n_words codewords by the law above, exactly
 * as stated, into out (word b at out + b*out_stride), record [n_words][3] and status [n_words];
 * each of the three may be NULL.  status_in [n_words] or NULL; with encode = 1 status_in, record
 * and status are ignored, and a code that is not encodable is SFE_ESTATE.  The reference of the
 * device's bytes.  Short strides are SFE_ERANGE. */
int sfe_dsp_ldpc_plan(int mb, int nb, int Z, const int16_t *shift, float scale, int a, int beta,
                      int max_iter, int in_mode, int skip, int encode, const void *in,
                      size_t in_stride, const int *status_in, size_t n_words, uint8_t *out,
                      size_t out_stride, uint32_t *record, int *status, int *n, int *k,
                      int *encodable);
/* Arguments are checked before the device is touched: SFE_EINVAL for a bad one on any machine,
 * SFE_ENODEV without a GPU.  shift is copied.  The parity part is inverted here, by elimination. */
int sfe_dsp_ldpc_create(int mb, int nb, int Z, const int16_t *shift, float scale, int a, int beta,
                        int max_iter, int in_mode, int skip, int device, sfe_ldpc_t *out);
/* n_words codewords each way.  d_status_in, d_rec and d_status may each be NULL.  *n_out = n_words;
 * n_words = 0 is a no-op.  A stride below what a codeword reads (n floats; skip + n or
 * skip + ceil(n / 2) symbols; ceil(k / 8) payload bytes) or writes (ceil(k / 8), ceil(n / 8)
 * bytes) is SFE_ERANGE; a null d_in, d_payload, d_bits or d_code, misaligned buffers (soft values,
 * records and statuses 4 bytes, symbols 8; payloads and codewords need none), n_words >= 2^31, a
 * stride that takes a buffer's byte range to 2^62, and any output byte range that overlaps an
 * input's or another output's are SFE_EINVAL, each with a message that starts with
 * "ldpc_process_stream: " or "ldpc_encode_stream: "; nothing is launched on a refusal.
 * Asynchronous on `stream`; one kernel launch and nothing else: allocates nothing, does not
 * synchronise the host, carries no state (there is no reset, and a handle has no setter), so a call
 * on a stream under graph capture IS supported. */
int sfe_dsp_ldpc_process_stream(sfe_ldpc_t h, const void *d_in, size_t in_stride,
                                const void *d_status_in, size_t n_words, void *d_bits,
                                size_t out_stride, void *d_rec, void *d_status, size_t *n_out,
                                sfe_stream_t stream);
int sfe_dsp_ldpc_encode_stream(sfe_ldpc_t h, const void *d_payload, size_t in_stride,
                               size_t n_words, void *d_code, size_t out_stride, size_t *n_out,
                               sfe_stream_t stream);
int sfe_dsp_ldpc_destroy(sfe_ldpc_t h);

/* ------------------------------------------------- OFDM burst receiver
 * The multicarrier answer to multipath, behind the correlator where sfe_dsp_burst_* stands on a
 * flat channel: for each burst a reach of T training and Ns data symbols of one stream, whose start
 * offset lies in device memory where sfe_dsp_corr_* wrote it, becomes Ns rows of Nd equalised
 * data-bin symbols -- cf32 whose components are the soft values sfe_dsp_vit_* and sfe_dsp_ldpc_*
 * read -- with a per-bin channel estimate, a record and a status.  Nothing is carried from burst to
 * burst; no host read or copy lies between the blocks.
 * Shape, fixed at create: n_fft = N a power of two in [64, 4096]; cp in [0, N]; advance = g in
 * [0, cp]: the transform window starts g samples before the end of the prefix; n_train = T in
 * [1, 4]; n_data = Ns in [1, 4096]; (T + Ns)(N + cp) < 2^31; kind [N] uint8 per FFT bin k: 0 null,
 * 1 data, 2 pilot, with Nd >= 1 data bins, Np >= 0 pilot bins, Nu = Nd + Np used bins; train [N]
 * cf32, finite, non-zero on every used bin; pilot [N] cf32 (may be NULL with Np = 0), finite,
 * non-zero on every pilot bin; pilot_sign [Ns] int8 of +-1, or NULL for all +1; cfo_mode 0 (none)
 * or 1 (from the cyclic prefix; needs cp >= 1); cfo_skip = q in [0, cp), 0 with cfo_mode 0;
 * out_mode SFE_OFDM_OUT_ZF or SFE_OFDM_OUT_MRC; min_gate finite; n_streams >= 1; anything else is
 * SFE_EINVAL with a message that starts with "ofdm: ".
 * Burst b of stream s starts at o = start_base + b*start_step + idx: the index and gate tables are
 * exactly sfe_dsp_burst_*'s, same layouts, same glue behind a one-template correlator.  Symbol j
 * in [0, T+Ns) occupies [o + j(N+cp), o + (j+1)(N+cp)); its window is the N samples from
 * o + j(N+cp) + cp - g.  With x stream s, float32 except where float64 is named:
 *   0  gate, range   as sfe_dsp_burst_*: status 2 for a gate value not >= min_gate; status 3 for a
 *                    reach [o, o + (T+Ns)(N+cp)) not inside [0, n_in).  Neither reads a sample.
 *   1  offset        cfo_mode 1: gamma = sum_{j<T+Ns} sum_{q<=i<cp} x[o+j(N+cp)+i+N]
 *                    conj(x[o+j(N+cp)+i]); eps = arg(gamma) / (2 pi) in subcarrier spacings,
 *                    |eps| <= 1/2.  Every sample of the reach is used as
 *                    x'[n] = x[o+n] exp(-j 2 pi eps n / N): the turn count is formed in float64 from
 *                    the float32 eps, reduced by rint, and only then taken to float32 (step 4 of
 *                    sfe_dsp_burst_*).  cfo_mode 0: eps = +0 and x' = x.
 *   2  transform     Y_j[k] = sum_{n<N} x'_j[n] exp(-j 2 pi k n / N), unscaled, over symbol j's
 *                    window.
 *   3  channel       H[k] = sum_{j<T} Y_j[k] c[k] on used bins, c[k] = conj(train[k]) /
 *                    (T |train[k]|^2) from a table made in float64 at create and rounded once;
 *                    h2 = (1/Nu) sum_used |H[k]|^2.
 *   4  common phase  per data symbol j < Ns: P_j = sum over the pilot bins k, increasing, of
 *                    Y_{T+j}[k] conj(H[k] pilot[k] pilot_sign[j]); phi_j = P_j / |P_j|, and
 *                    1 + 0j when Np = 0.
 *   5  output        for the data bins in increasing k, i = 0 .. Nd-1:
 *                    ZF   Z = Y_{T+j}[k] conj(H[k] phi_j) / |H[k]|^2;
 *                    MRC  Z = Y_{T+j}[k] conj(H[k] phi_j) / h2, the matched-filter output: a QPSK or
 *                         BPSK soft value up to one scale per burst, which is what min-sum and
 *                         Viterbi need;
 *                    cf32 at d_out + (s*n_bursts + b)*out_stride + j*Nd + i.  With d_chan, H as N
 *                    cf32 at d_chan + (s*n_bursts + b)*N, unused bins +0.  The record, 8 float32 at
 *                    d_rec + (s*n_bursts + b)*8: eps; h2; min_used |H|^2 / h2; the pilot error
 *                    sum_j sum_pilot |Y conj(H phi_j) / |H|^2 - pilot sign|^2 / sum_j sum_pilot
 *                    |pilot|^2 (+0 with Np = 0); arg(phi_0) / (2 pi); arg(phi_{Ns-1}) / (2 pi); +0;
 *                    +0.  The status, int32 at d_status + s*status_stride + b: 0.
 *   6  failure       status 1 for a non-finite sample in the reach, a gamma that is zero or not
 *                    finite in cfo_mode 1, a used bin whose |H|^2 is zero or not finite, or a P_j
 *                    that is zero or not finite with Np > 0.  A burst of status 1, 2 or 3 gets Ns Nd
 *                    symbols of +0, a d_chan row of +0 and a record of quiet NaN whose words 6 and
 *                    7 are still +0.
 * Promised: the same call gives the same bits on every run; a burst's output depends on its reach,
 * the handle and the parameters only -- never on b, s, n_bursts, addresses, strides, whether
 * windows overlap (they may) or how the kernel splits a burst over workgroups; u8 input gives the
 * bits of the cf32 path on the converted samples; nothing outside the slots named is written; the
 * exact case: with cfo_mode 0, Np = 0, T = 1, train all ones and x = 1+0j at every window's first
 * sample and +0 elsewhere, every Z is exactly 1+0j in both output modes, H is exactly 1+0j on used
 * bins and h2 is 1.  Not promised: the order of the sums, equal bits between shapes, the bits of
 * the host plan. */
#define SFE_OFDM_OUT_ZF 0
#define SFE_OFDM_OUT_MRC 1
typedef void *sfe_ofdm_t;   /* opaque: one receiver over n_streams streams */
/* Host-only (no GPU): validates what create validates (one stream).  With x != NULL -- n_in cf32
 * samples of ONE stream -- it runs n_bursts bursts by the law in float64 (idx [n_bursts] and gate
 * [n_bursts] host arrays, either may be NULL), eps, H and phi_j rounded to float32 where the law
 * hands them on, and rounds once to float32 into symbols [n_bursts][Ns*Nd] cf32 (required then),
 * chan [n_bursts][N] cf32, record [n_bursts][8] and status [n_bursts] (each may be NULL): the CPU
 * fallback, and the reference of the device's values (not of its bits).  n_in or n_bursts >= 2^31,
 * or a start_base + b*start_step beyond +-(2^63 - 2^33) for some burst, is SFE_EINVAL. */
int sfe_dsp_ofdm_plan(int n_fft, int cp, int advance, int n_train, int n_data, const uint8_t *kind,
                      const float *train, const float *pilot, const int8_t *pilot_sign,
                      int cfo_mode, int cfo_skip, int out_mode, float min_gate, const float *x,
                      size_t n_in, const uint32_t *idx, const float *gate, size_t n_bursts,
                      int64_t start_base, int64_t start_step, float *symbols, float *chan,
                      float *record, int *status);
/*   kind, train, pilot, pilot_sign   copied
 * Arguments are checked before the device is touched: SFE_EINVAL for a bad one on any machine,
 * SFE_ENODEV without a GPU. */
int sfe_dsp_ofdm_create(int n_fft, int cp, int advance, int n_train, int n_data,
                        const uint8_t *kind, const float *train, const float *pilot,
                        const int8_t *pilot_sign, int cfo_mode, int cfo_skip, int out_mode,
                        float min_gate, int n_streams, int device, sfe_ofdm_t *out);
/* SFE_FMT_F32 (cf32 input, 8-byte aligned) or SFE_FMT_U8 ((I,Q) byte pairs, 2-byte aligned,
 * converted (b-128)*(1/127) on load exactly as sfe_dsp_rx_u8_to_f32); any other format is
 * SFE_EINVAL.  A call takes the format by value when it is enqueued. */
int sfe_dsp_ofdm_set_input_format(sfe_ofdm_t h, int fmt);
/* n_bursts bursts of every stream: stream s at d_in + s*in_stride (samples of the input format),
 * n_in samples long; the other layouts as above.  d_idx, d_gate, d_chan, d_rec and d_status may
 * each be NULL.  *n_out = n_bursts; n_bursts = 0 is a no-op.  out_stride < Ns*Nd, or status_stride
 * < n_bursts with d_status, is SFE_ERANGE; a null d_in or d_out, misaligned buffers (cf32 8 bytes,
 * u8 pairs 2, the rest 4), in_stride < n_in with more than one stream, n_in >= 2^31,
 * n_streams*n_bursts >= 2^31, a start_base + b*start_step beyond +-(2^63 - 2^33) for some burst, a
 * stride that takes a buffer's byte range to 2^62 and any output byte range that overlaps the
 * input's, the index table's, the gate table's or another output's are SFE_EINVAL; every refusal
 * carries a message that starts with "ofdm_process_stream: " and nothing is launched.
 * Asynchronous on `stream`; one kernel launch and nothing else: allocates nothing, does not
 * synchronise the host, carries no state (there is no reset).  The handle has no setter apart from
 * the input format, which the call takes by value, so a call on a stream under graph capture IS
 * supported. */
int sfe_dsp_ofdm_process_stream(sfe_ofdm_t h, const void *d_in, size_t n_in, size_t in_stride,
                                const void *d_idx, size_t idx_stride, const void *d_gate,
                                size_t gate_stride, size_t n_bursts, int64_t start_base,
                                int64_t start_step, void *d_out, size_t out_stride, void *d_chan,
                                void *d_rec, void *d_status, size_t status_stride, size_t *n_out,
                                sfe_stream_t stream);
int sfe_dsp_ofdm_destroy(sfe_ofdm_t h);

/* ------------------------------------------------- OFDM burst modulator
 * The transmit mirror of the OFDM burst receiver: per burst, a row of coded bits -- what
 * sfe_dsp_ldpc_encode_stream, sfe_dsp_vit_* or sfe_dsp_reed_* wrote -- or of cf32 symbols -- a row
 * of sfe_dsp_ofdm_*'s d_out -- on the device becomes one frame of T training and Ns data symbols,
 * each N samples behind its cyclic prefix, at a stated place of an output stream, cf32 or the
 * transmit wire format.  Bursts and symbols are independent; nothing is carried.  No NCO: frequency
 * placement is sfe_dsp_combine_*'s.
 * Shape, fixed at create: n_fft = N, cp, n_train = T, n_data = Ns, kind [N], train [N], pilot [N]
 * and pilot_sign [Ns] mean what they mean for sfe_dsp_ofdm_* and are validated the same way: N a
 * power of two in [64, 4096]; cp in [0, N]; T in [1, 4]; Ns in [1, 4096]; (T + Ns)(N + cp) < 2^31;
 * Nd >= 1 data bins; train finite, and non-zero on every used bin; pilot (may be NULL with Np = 0)
 * finite, and non-zero on every pilot bin; pilot_sign of +-1, or NULL for all +1.  There is no
 * advance, cfo or out_mode.  amp is finite and > 0; order is 2 or 4; in_mode is
 * SFE_OFDMMOD_IN_BITS or SFE_OFDMMOD_IN_SYMBOLS; out_fmt is SFE_FMT_F32 or SFE_FMT_TX10, under
 * which cp must be even.  There is no setter.  Anything else is SFE_EINVAL with a message that
 * starts with "ofdmmod: ".
 * Bins: two tables are made at create, ta = amp train and pa = amp pilot, one float32 product per
 * component.  For symbol j < T + Ns and bin k: a null bin is +0; a training symbol (j < T) carries
 * ta[k] on every used bin; a data symbol carries pa[k] pilot_sign[j-T], one product per component,
 * on a pilot bin, and on data bin i of Nd, in increasing k:
 *   BITS, order 2      (amp (1 - 2c), +0)
 *   BITS, order 4      (a4 (1 - 2 c_0), a4 (1 - 2 c_1)), a4 = float32(amp / sqrt 2), formed in
 *                      float64 and rounded once: sfe_dsp_mod_*'s Gray QPSK, which SFE_VIT_IN_QPSK
 *                      undoes
 *                      coded bit t = ((j-T) Nd + i) bps + c, bps = 1 or 2, is bit 7 - (t mod 8) of
 *                      byte floor(t / 8) at d_in + b*in_stride (bytes): MSB-first, the layout
 *                      sfe_dsp_ldpc_encode_stream, sfe_dsp_vit_* and sfe_dsp_reed_* write.  A burst
 *                      reads ceil(Ns Nd bps / 8) bytes.
 *   SYMBOLS            the cf32 at d_in + b*in_stride + (j-T) Nd + i (in_stride in cf32) times amp,
 *                      one product per component; order is ignored.  Exactly the layout of
 *                      sfe_dsp_ofdm_*'s d_out rows; a burst reads Ns Nd cf32.
 * Transform: x_j[n] = (1/N) sum_k X_j[k] exp(+j 2 pi k n / N), so that the receiver's H is the
 * channel's response.  simplefe_amd/csrc/ofdmmod_law.h states it operation by operation, and both
 * the kernel and the host plan compile that header: one radix-2 pass when log2 N is odd, then
 * radix-4 Stockham passes; twiddles from a table exp(+j 2 pi q / N) made in float64 and rounded
 * once; the complex product two explicit fmaf over one rounded product each; every output of a
 * pass a fixed expression of its inputs; last the product with the exact power of two 1/N.  Passes
 * are data-parallel, so no order of lanes can matter.
 * Frame: symbol j is cp + N samples, x_j[N-cp .. N) then x_j[0 .. N); F = (T + Ns)(N + cp).
 * Placement: sfe_dsp_mod_*'s, word for word.  A call defines EVERY sample of the output stream
 * [0, n_out).  Burst b's frame occupies [o_b, o_b + F), o_b = start_base + b*start_step; every
 * sample in no frame is +0.  SFE_EINVAL, nothing launched: start_base < 0; start_step < F with
 * more than one burst (start_step is ignored with one); o_(n_bursts-1) + F > n_out; n_out or
 * n_bursts >= 2^31; an odd n_out under TX10.  n_bursts = 0 writes n_out zeros.
 * TX10: the bytes are exactly sfe_dsp_tx_f32_to_10bit's of the F32 output -- two complex samples in
 * 5 bytes, the groups aligned to the stream; (n_out / 2) * 5 bytes are written.  In addition cp
 * (at create), start_base and start_step (at the call; start_step with more than one burst) must
 * be even, so that no group straddles a symbol or a frame: an odd one is SFE_EINVAL.  A call whose
 * workgroups -- one per symbol, one per 4096 samples in no frame -- number 2^31 or more is
 * SFE_EINVAL.
 * Promised: the same call gives the same bits on every run; a frame depends on its input row and
 * the handle only -- never on b, n_bursts, addresses, strides or offsets; the device's F32 words
 * and TX10 bytes EQUAL sfe_dsp_ofdmmod_plan's, for every input whose intermediate values are zero
 * or normal numbers (nothing is promised otherwise); nothing outside the n_out samples is written;
 * samples i and i + N of a symbol are bit-equal for i < cp; the exact case: with every bin a data
 * bin, order 2, amp 1 and all bits 0, a data symbol is exactly 1+0j at its sample cp and zero at
 * every other sample (compare with ==: the sign of a zero is not promised; with cp = N the prefix
 * is the whole symbol, so sample 0 is the copy of sample cp), and with train all ones so is a
 * training symbol -- the input of sfe_dsp_ofdm_*'s own exact case with advance 0.
 * There is no status output: bytes are always valid, and a non-finite symbol in SYMBOLS mode
 * propagates (nothing is promised for it). */
#define SFE_OFDMMOD_IN_BITS 0
#define SFE_OFDMMOD_IN_SYMBOLS 1
typedef void *sfe_ofdmmod_t;  /* opaque: one modulator; it owns its tables on the device and nothing in it changes after create */
/* Host-only: the lanes of the workgroup that makes one symbol of n_fft bins, the samples in no
 * frame one workgroup writes, and the LDS a symbol's workgroup uses (each pointer may be NULL). */
int sfe_dsp_ofdmmod_footprint(int n_fft, int *threads, int *zero_tile_samples, size_t *lds_bytes);
/* Host-only (no GPU): validates what create validates and reports Nd, F and what a burst reads --
 * bytes in BITS mode, cf32 symbols in SYMBOLS mode (each pointer may be NULL); then the placement
 * as process_stream does; then, with out != NULL, writes the stream by the law above, exactly as
 * stated -- n_out cf32 samples, or (n_out / 2) * 5 bytes under SFE_FMT_TX10 -- from in (host
 * memory laid out as d_in; required with n_bursts > 0): the reference of the device's bits.
 * in_stride below what a burst reads is SFE_ERANGE. */
int sfe_dsp_ofdmmod_plan(int n_fft, int cp, int n_train, int n_data, const uint8_t *kind,
                         const float *train, const float *pilot, const int8_t *pilot_sign,
                         float amp, int order, int in_mode, int out_fmt, const void *in,
                         size_t in_stride, size_t n_bursts, int64_t start_base, int64_t start_step,
                         size_t n_out, void *out, int *n_data_bins, int *frame_len, size_t *n_in);
/*   kind, train, pilot, pilot_sign   copied
 * Arguments are checked before the device is touched: SFE_EINVAL for a bad one on any machine,
 * SFE_ENODEV without a GPU. */
int sfe_dsp_ofdmmod_create(int n_fft, int cp, int n_train, int n_data, const uint8_t *kind,
                           const float *train, const float *pilot, const int8_t *pilot_sign,
                           float amp, int order, int in_mode, int out_fmt, int device,
                           sfe_ofdmmod_t *out);
/* One stream of n_out samples holding n_bursts frames.  *n_written = n_out.  The placement
 * refusals above; in_stride below what a burst reads is SFE_ERANGE; a null d_out, a null d_in with
 * bursts, a cf32 d_out or a cf32 d_in (SYMBOLS mode) that is not 8-byte aligned (TX10 output and
 * coded bytes need no alignment), an in_stride that takes the input's byte range to 2^62 and an
 * output byte range that overlaps the input's are SFE_EINVAL; every refusal carries a message that
 * starts with "ofdmmod_process_stream: " and nothing is launched.  n_out = 0 is a no-op.
 * Asynchronous on `stream`; one kernel launch and nothing else: allocates nothing, does not
 * synchronise the host, carries no state (there is no reset).  A handle has no setter, so a call
 * on a stream under graph capture IS supported.  Behind sfe_dsp_ldpc_encode_stream its d_out and
 * out_stride, behind sfe_dsp_ofdm_* its d_out and out_stride (a non-regenerative relay), are the
 * whole glue. */
int sfe_dsp_ofdmmod_process_stream(sfe_ofdmmod_t h, const void *d_in, size_t in_stride,
                                   size_t n_bursts, int64_t start_base, int64_t start_step,
                                   void *d_out, size_t n_out, size_t *n_written,
                                   sfe_stream_t stream);
int sfe_dsp_ofdmmod_destroy(sfe_ofdmmod_t h);

/* ------------------------------------------------- QAM mapper and soft demapper
 * One handle, two directions, like sfe_dsp_reed_* and sfe_dsp_ldpc_*.  map: rows of coded bytes on
 * the device -- what sfe_dsp_ldpc_encode_stream, sfe_dsp_vit_* or sfe_dsp_reed_* wrote -- become
 * rows of cf32 constellation points, laid out as sfe_dsp_ofdmmod_*'s SYMBOLS mode reads them.
 * demap: rows of cf32 equalised symbols, laid out as sfe_dsp_ofdm_* writes them, become rows of
 * float32 max-log LLRs, laid out as SFE_VIT_IN_SOFT of sfe_dsp_ldpc_* and sfe_dsp_vit_* reads them,
 * each symbol weighted, where the handle says so, by |H|^2 read from sfe_dsp_ofdm_*'s d_chan where
 * it lies.  Both directions take an optional bit interleaver per row.  Rows are independent;
 * nothing is carried.
 * Shape, fixed at create: order M in {2, 4, 16, 64, 256}, bps = log2 M; amp finite and > 0; scale
 * finite and > 0; n_sym in [1, 2^24] symbols per row, B = n_sym bps bits per row; perm [B] uint32,
 * a permutation of [0, B) validated at create, or NULL for the identity; csi_period in [0, 4096],
 * 0 for no channel weighting, else csi_len in [1, 65536] and csi_index [csi_period] uint32, each
 * < csi_len (behind sfe_dsp_ofdm_*: csi_period = Nd, csi_len = N, csi_index[i] = the FFT bin of
 * data bin i).  There is no setter and no state.  Anything else is SFE_EINVAL with a message that
 * starts with "qam: ", on any machine, before the device is touched.
 * Constellation: an axis carries m bits, m = bps / 2 for M >= 4; for M = 2, m = 1 on I only, Q is
 * +0 on map and ignored on demap.  The axis word w = (b_0 .. b_(m-1)), b_0 first (as a number: b_0
 * its most significant bit), has the odd integer u(w) = (1 - 2 b_0) A(b_1 ..), A() = 1,
 * A(b, rest) = 2^(len(rest)+1) - (1 - 2b) A(rest): Gray along the axis, b_0 = 0 the positive half;
 * for m = 2 the words 11, 10, 00, 01 stand at -3, -1, +1, +3.  The level table is
 * lev[w] = float32(amp d_M u(w)), d_2 = 1 and d_M = sqrt(3 / (2 (M - 1))) = 1 / sqrt(K_M) with the
 * integer K_M = 2 (M - 1) / 3 (2, 10, 42, 170) for M >= 4: formed in float64 from the float32 amp
 * as amp u(w) / sqrt(K_M) and rounded once, so that M = 4 is exactly sfe_dsp_mod_*'s and
 * sfe_dsp_ofdmmod_*'s Gray QPSK.  At most 16 entries, made at create.
 * Bits: symbol q of a row carries the symbol-bit positions t = q bps + c, c < bps: c < m is I-axis
 * bit c, c >= m is Q-axis bit c - m.  Position t holds coded bit perm[t].  Coded bit v is bit
 * 7 - (v mod 8) of byte floor(v / 8) of the row: MSB-first, the layout
 * sfe_dsp_ldpc_encode_stream, sfe_dsp_vit_* and sfe_dsp_reed_* write.  A row reads ceil(B / 8)
 * bytes.
 * Map: the cf32 at d_sym + row*out_stride + q is (lev[w_I], lev[w_Q]): table words.
 * Demap, stated operation by operation in simplefe_amd/csrc/qam_law.h, which the kernel and the
 * host plan both compile, every operation one IEEE float32 operation and nothing contracted.  For
 * the symbol z at d_sym + row*in_stride + q:
 *   weight   no CSI: w = scale.  CSI: h = d_csi[row*csi_stride + csi_index[q mod csi_period]],
 *            g = fmaf(h.i, h.i, h.r h.r), w = scale g.
 *   per axis value y (z.r or z.i) and axis bit c: for every word v, e_v = t t with t = y - lev[v];
 *            D0 = min of e_v over the words whose bit c is 0, D1 over those whose bit c is 1 (min
 *            is exact, so its order cannot show); r = w (D1 - D0).  r > 0 favours bit 0: the sign
 *            of sfe_dsp_vit_* and sfe_dsp_ldpc_*.
 *   store    r as float32 at d_soft + row*out_stride + perm[t].
 * Promised: the same call gives the same bits on every run; a row's output depends on that row,
 * its csi row and the handle only -- never on the row number, the count, addresses or strides; the
 * device's words EQUAL sfe_dsp_qam_plan's for every input whose intermediate values are zero or
 * normal numbers (otherwise the words are written and nothing is said of them); exactly the B
 * floats (demap) or n_sym cf32 (map) of each row are written, nothing between rows, to the byte;
 * the exact case: order 2, amp 1, scale 1, no CSI, the symbol 0.5+0j gives r exactly 2. */
#define SFE_QAM_MAP 0
#define SFE_QAM_DEMAP 1
typedef void *sfe_qam_t;  /* opaque: one mapper / demapper; it owns its tables on the device and nothing in it changes after create */
/* Host-only (no GPU): validates what create validates and reports bps and the bytes a row of
 * coded bits holds, ceil(B / 8) (each pointer may be NULL); then, with in != NULL, runs n_rows rows
 * by the law above into out, exactly as stated: the reference of the device's bits.  direction
 * SFE_QAM_MAP: in is bytes (in_stride in bytes), out cf32 (out_stride in cf32), csi is ignored.
 * SFE_QAM_DEMAP: in is cf32 (in_stride in cf32), csi cf32 rows at csi_stride (required exactly
 * when csi_period > 0), out float32 (out_stride in floats).  Host buffers need no alignment.  A
 * stride below its row (ceil(B / 8) bytes, n_sym cf32, csi_len cf32, B floats) is SFE_ERANGE. */
int sfe_dsp_qam_plan(int order, float amp, float scale, size_t n_sym, const uint32_t *perm,
                     int csi_period, int csi_len, const uint32_t *csi_index, int direction,
                     const void *in, size_t in_stride, const void *csi, size_t csi_stride,
                     size_t n_rows, void *out, size_t out_stride, int *bps, size_t *row_bytes);
/*   perm, csi_index   copied
 * Arguments are checked before the device is touched: SFE_EINVAL for a bad one on any machine,
 * SFE_ENODEV without a GPU. */
int sfe_dsp_qam_create(int order, float amp, float scale, size_t n_sym, const uint32_t *perm,
                       int csi_period, int csi_len, const uint32_t *csi_index, int device,
                       sfe_qam_t *out);
/* Row r reads ceil(B / 8) bytes at d_bytes + r*in_stride (bytes) and writes n_sym cf32 at
 * d_sym + r*out_stride (cf32).  *n_out = n_rows; n_rows = 0 is a no-op.  A stride below its row
 * is SFE_ERANGE; a null buffer, a d_sym that is not 8-byte aligned (coded bytes need no
 * alignment), n_rows >= 2^31, a stride that takes a buffer's byte range to 2^62, a call of 2^31
 * workgroups or more (one per 2048 symbols of a row) and an output byte range that overlaps the
 * input's are SFE_EINVAL; every refusal carries a message that starts with "qam_map_stream: " and
 * nothing is launched.  Asynchronous on `stream`; one kernel launch and nothing else: allocates
 * nothing, does not synchronise the host, and may be captured into a graph.  Behind
 * sfe_dsp_ldpc_encode_stream its d_code and out_stride, in front of sfe_dsp_ofdmmod_* (SYMBOLS
 * mode, whose amp then multiplies) its d_in and in_stride, are the whole glue. */
int sfe_dsp_qam_map_stream(sfe_qam_t h, const void *d_bytes, size_t in_stride, size_t n_rows,
                           void *d_sym, size_t out_stride, size_t *n_out, sfe_stream_t stream);
/* Row r reads n_sym cf32 at d_sym + r*in_stride (cf32) and, on a handle with csi_period > 0,
 * csi_len cf32 at d_csi + r*csi_stride (cf32); it writes B floats at d_soft + r*out_stride
 * (floats).  d_csi is required exactly when the handle has csi_period > 0 and refused otherwise.
 * *n_out = n_rows; n_rows = 0 is a no-op.  A stride below its row is SFE_ERANGE; a null buffer,
 * misaligned buffers (cf32 8 bytes, floats 4), n_rows >= 2^31, a stride that takes a buffer's
 * byte range to 2^62, a call of 2^31 workgroups or more and an output byte range that overlaps an
 * input's are SFE_EINVAL; every refusal carries a message that starts with "qam_demap_stream: "
 * and nothing is launched.  Asynchronous, one launch, no allocation, no host synchronisation,
 * capturable.  Behind sfe_dsp_ofdm_* (zero-forcing output) its d_out, out_stride, d_chan and
 * n_fft, in front of sfe_dsp_ldpc_* or sfe_dsp_vit_* (SFE_VIT_IN_SOFT) their d_in and in_stride,
 * are the whole glue. */
int sfe_dsp_qam_demap_stream(sfe_qam_t h, const void *d_sym, size_t in_stride, const void *d_csi,
                             size_t csi_stride, size_t n_rows, void *d_soft, size_t out_stride,
                             size_t *n_out, sfe_stream_t stream);
int sfe_dsp_qam_destroy(sfe_qam_t h);

/* ------------------------------------------------- 2-(G)FSK burst modem
 * One handle, two directions, like sfe_dsp_qam_*.  mod: per burst, ceil(n_bits / 8) coded bytes on
 * the device -- what sfe_dsp_ldpc_encode_stream, sfe_dsp_vit_* or sfe_dsp_reed_* wrote -- become
 * one continuous-phase, constant-envelope frame behind a preamble, placed in an output stream as
 * sfe_dsp_mod_* places its frames.  demod: per burst, a window of a stream that starts where
 * sfe_dsp_corr_*'s peak says goes through a quadrature discriminator and a matched filter; timing,
 * deviation and carrier offset are fitted on the preamble, and the data symbols come out as float32
 * soft values (positive for bit 0, the sign of sfe_dsp_vit_* and sfe_dsp_ldpc_*) and, where asked,
 * as packed hard bits (what sfe_dsp_reed_* and this block's mod read).  Nothing is carried.  M = 2
 * only: 4-level FSK needs a sequence detector and is not built.
 * Shape, fixed at create: sps in [2, 64]; the frequency pulse g [n_taps] real float32, finite,
 * 1 <= n_taps <= 64 sps, Q = ceil(n_taps / sps); the modulation index h finite and > 0; amp finite
 * and > 0; preamble bits pre [n_pre = Lp] bytes of 0 or 1, Lp in [2, 1024]; n_bits in [1, 32768];
 * N = Lp + n_bits symbols; the matched filter m [n_mf] real float32, finite, n_mf in [1, 256], its
 * sum (formed in float64) > 0; delay in [1, 2^20]; the timing range R in [0, 64]; scale finite and
 * > 0; min_gate finite; n_streams >= 1; out_fmt SFE_FMT_F32 or SFE_FMT_TX10.  Anything else is
 * SFE_EINVAL with a message that starts with "fsk: ", on any machine, before the device is touched.
 * The law is stated operation by operation in simplefe_amd/csrc/fsk_law.h, which the kernels and
 * the host plan both compile: every multiply that feeds an add an explicit fmaf, everything else
 * one IEEE float32 operation or exact integer arithmetic mod 2^32 as uint32, nothing contracted.
 * A symbol's level is a = 1 - 2c for its bit c.
 * Integer phase: G[j] = rint(h g[j] 2^31), formed in float64 and rounded once; C[0] = 0,
 * C[j+1] = C[j] + G[j], Gsum = C[n_taps].  Create refuses a sum of the G that is <= 0 as a signed
 * sum, and any residue r with sum over q of |G[q sps + r]| >= 2^30: that sum is the instantaneous
 * frequency, kept under a quarter turn per sample so that the discriminator has room for a carrier
 * offset.  A frame has F = (N + Q - 1) sps + 1 samples -- the last symbol's last phase increment
 * ends on the final one -- and P[i] = sum over k < N of a_k C[clamp(i - k sps, 0, n_taps)], exact,
 * so the order of summation cannot show.
 * fsk_cis(p): q = ((p + 2^29) >> 30) & 3, r = (int32)(p - (q << 30)) in [-2^29, 2^29),
 * t = (float)r 2^-29, z = t t; s = t S(z), c = 1 + z Cc(z) by fmaf chains (four coefficients each,
 * the last constant of the cosine's chain exactly 1); rotated by q: (c, s), (-s, c), (-c, -s),
 * (s, -c).  fsk_cis(k 2^30) is exactly (+-1, +-0) or (+-0, +-1), and each component is within
 * 2 ulp(1) = 2.39e-7 of float64 cos / sin for every one of the 2^32 phases.
 * Modulator: y[i] = (amp c, amp s) of fsk_cis(P[i]), one product per component.  Payload bit t of
 * burst b is bit 7 - (t mod 8) of byte floor(t / 8) at d_bytes + b*in_stride: MSB-first; pad bits
 * are ignored.  Placement is sfe_dsp_mod_*'s with this F: a call defines every sample of
 * [0, n_out), a sample in no frame is +0, the refusals for start_base, start_step and n_out are
 * the same.  TX10 bytes are exactly sfe_dsp_tx_f32_to_10bit's of the F32 output, groups aligned to
 * the stream, not to frames.
 * Demodulator: burst b of stream s starts at o = start_base + b*start_step + idx; d_idx, d_gate
 * and statuses 2 and 3 are sfe_dsp_burst_*'s.
 *   reach    [o + delay - R - 1, o + delay + R + (N - 1) sps + n_mf) of the stream's samples; not
 *            inside [0, n_in): status 3.  A gate below min_gate, or a NaN gate: status 2.  Neither
 *            reads a sample.
 *   v        v[i] = the FM detector of sfe_dsp_polar_* (polar_law.h, gain 1) of x[o + i] and its
 *            predecessor; u8 input is converted as sfe_dsp_rx_u8_to_f32 converts it.
 *   u        u(i) = sum over j < n_mf of m[j] v[i + j], an fmaf chain from +0 in increasing j.
 *   e        the expected response of the preamble, made at create in float64 from the integer
 *            pulse so that inter-symbol interference inside the preamble does not bias the fit:
 *            D[i] = sum over k < Lp of a_k G[i - k sps] (data symbols taken as 0),
 *            U = (sum of G / sps) sum m, e[k] = float32(sum_j m[j] D[delay + k sps + j - 1] / U);
 *            se = sum e, see = sum e^2, den = Lp see - se^2 formed in float64 and rounded once;
 *            create refuses den not > 0.  A long run of one level then reads w = a.
 *   fit      for tau = -R .. R, u_k = u(delay + tau + k sps), S1 = sum u_k and Se = sum e_k u_k
 *            (the products rounded first), both PAIRWISE TREES: padded with +0 to the next power
 *            of two, at each level s[k] = s[2k] + s[2k+1].  num = fmaf((float)Lp, Se, -(se S1)).
 *            tau^ is the tau of the greatest num, the lowest among equals; a NaN never wins.
 *            dev = num / den, dc = (S1 - dev se) / (float)Lp, f = dc 0x1.45f306p-3f in turns per
 *            sample.  The residual is the same tree over (u_k - fmaf(dev, e_k, dc))^2 and
 *            q = resid / ((dev dev) see).
 *   output   for k = Lp .. N - 1: w = (u(delay + tau^ + k sps) - dc) / dev, r = scale w, float32 at
 *            d_soft + (s*n_bursts + b)*soft_stride + (k - Lp).  With d_bits, bit (r < 0) is packed
 *            MSB-first into ceil(n_bits / 8) bytes at d_bits + (s*n_bursts + b)*bits_stride, pad
 *            bits 0.  The record is 8 float32: tau^, f, dev, q, then +0 four times.  Status 0.
 *   failure  status 1: a non-finite sample in the reach, every num NaN, or a dev that is not > 0
 *            and finite.  For status 1, 2 or 3 the soft values are +0, the bytes 0, the record
 *            quiet NaN in words 0-3 and +0 in words 4-7.
 * Promised: the same call gives the same bits on every run; a frame depends on its bytes and the
 * handle only; a burst's outputs depend on its reach and the handle only -- never on b, s,
 * n_bursts, addresses, strides or overlapping windows; u8 input gives the bits of the cf32 path on
 * the converted samples; the device's F32 words, TX10 bytes, soft values, packed bits, records and
 * statuses EQUAL sfe_dsp_fsk_plan's for every finite input whose partial sums are zero or normal
 * numbers; nothing outside the named slots is written. */
#define SFE_FSK_MOD 0
#define SFE_FSK_DEMOD 1
typedef void *sfe_fsk_t;  /* opaque: one modem; it owns its tables on the device and nothing in it changes after create but the input format */
/* Host-only (no GPU): validates what create validates and reports N, F, e [n_pre] and den (each
 * pointer may be NULL); then runs one direction by the law above, exactly as stated: the reference
 * of the device's bits.  SFE_FSK_MOD: in is the payload bytes, in_len their stride in bytes
 * (SFE_ERANGE below ceil(n_bits / 8)); out is the whole stream of n_out samples, cf32 or TX10
 * groups; the placement is checked even without out.  SFE_FSK_DEMOD: in is ONE stream of in_len
 * cf32 samples; idx and gate are host arrays of n_bursts entries or NULL; out takes n_bits float32
 * per burst, bits (or NULL) ceil(n_bits / 8) bytes per burst, record (or NULL) 8 float32 per burst,
 * status (or NULL) one int per burst, all contiguous; n_out is ignored. */
int sfe_dsp_fsk_plan(int sps, const float *pulse, int n_taps, float h, float amp,
                     const uint8_t *pre, int n_pre, int n_bits, const float *mf, int n_mf,
                     int delay, int range, float scale, float min_gate, int out_fmt, int direction,
                     const void *in, size_t in_len, const uint32_t *idx, const float *gate,
                     size_t n_bursts, int64_t start_base, int64_t start_step, void *out,
                     size_t n_out, uint8_t *bits, float *record, int *status, int *n_sym,
                     int *frame_len, float *e, float *den);
/*   pulse, pre, mf   copied
 * Arguments are checked before the device is touched: SFE_EINVAL for a bad one on any machine,
 * SFE_ENODEV without a GPU. */
int sfe_dsp_fsk_create(int sps, const float *pulse, int n_taps, float h, float amp,
                       const uint8_t *pre, int n_pre, int n_bits, const float *mf, int n_mf,
                       int delay, int range, float scale, float min_gate, int out_fmt,
                       int n_streams, int device, sfe_fsk_t *out);
/* The demodulator's input: SFE_FMT_F32 (cf32, the default) or SFE_FMT_U8 ((I,Q) byte pairs).
 * Takes effect from the next call; a captured call keeps the format it was captured with.  It is
 * the handle's only setter. */
int sfe_dsp_fsk_set_input_format(sfe_fsk_t h, int fmt);
/* Burst b reads ceil(n_bits / 8) bytes at d_bytes + b*in_stride (bytes) and its F samples start at
 * sample start_base + b*start_step of the n_out samples at d_out (cf32, or 5-byte groups of two
 * samples with SFE_FMT_TX10); the call writes all n_out samples.  *n_written = n_out.  The checks
 * and their codes are sfe_dsp_mod_process_stream's, word for word, with the prefix
 * "fsk_mod_stream: "; nothing is launched on a refusal.  Asynchronous on `stream`; one kernel
 * launch and nothing else: allocates nothing, does not synchronise the host, carries no state, and
 * may be captured into a graph.  Behind sfe_dsp_ldpc_encode_stream or sfe_dsp_reed_* their output
 * and its stride are the whole glue. */
int sfe_dsp_fsk_mod_stream(sfe_fsk_t h, const void *d_bytes, size_t in_stride, size_t n_bursts,
                           int64_t start_base, int64_t start_step, void *d_out, size_t n_out,
                           size_t *n_written, sfe_stream_t stream);
/* Stream s is the n_in samples at d_in + s*in_stride (samples of the input format); d_idx (uint32,
 * + s*idx_stride + b), d_gate (float32, + s*gate_stride + b), d_bits, d_rec (+ (s*n_bursts + b)*8
 * float32) and d_status (int32, + s*status_stride + b) may each be NULL.  *n_out = n_bursts;
 * n_bursts = 0 is a no-op.  soft_stride < n_bits, bits_stride < ceil(n_bits / 8) (with d_bits) and
 * status_stride < n_bursts (with d_status) are SFE_ERANGE; a null d_in or d_soft, misaligned
 * buffers (cf32 8 bytes, u8 pairs 2, the 4-byte kinds 4; packed bits need none), n_in >= 2^31,
 * n_streams * n_bursts >= 2^31, in_stride < n_in with several streams, starts that leave int64, a
 * stride that takes a buffer's byte range to 2^62, and outputs that overlap an input or one
 * another are SFE_EINVAL; every refusal carries a message that starts with "fsk_demod_stream: "
 * and nothing is launched.  Asynchronous, one launch, no allocation, no host synchronisation, no
 * state, capturable.  Behind sfe_dsp_corr_* (one template: the plan's modulated preamble)
 * d_peak_idx and d_peak_val as they lie are d_idx and d_gate, and start_step is the correlator's
 * block; in front of sfe_dsp_vit_* or sfe_dsp_ldpc_* (SFE_VIT_IN_SOFT) d_soft and soft_stride, in
 * front of sfe_dsp_reed_* d_bits and bits_stride, are the whole glue. */
int sfe_dsp_fsk_demod_stream(sfe_fsk_t h, const void *d_in, size_t n_in, size_t in_stride,
                             const void *d_idx, size_t idx_stride, const void *d_gate,
                             size_t gate_stride, size_t n_bursts, int64_t start_base,
                             int64_t start_step, void *d_soft, size_t soft_stride, void *d_bits,
                             size_t bits_stride, void *d_rec, void *d_status, size_t status_stride,
                             size_t *n_out, sfe_stream_t stream);
int sfe_dsp_fsk_destroy(sfe_fsk_t h);

/* ------------------------------------------------- frame check: CRC and scrambler
 * What answers "is this payload the one that was sent": on transmit, in front of sfe_dsp_reed_*'s
 * encoder, sfe_dsp_mod_*, sfe_dsp_ldpc_encode_stream or sfe_dsp_fsk_mod_stream, rows of P payload
 * bytes become rows of Fb = P + w/8 frame bytes -- the payload, its CRC, and the whole frame XOR a
 * PN sequence (append); on receive, behind sfe_dsp_vit_*, sfe_dsp_reed_process_stream,
 * sfe_dsp_ldpc_* or sfe_dsp_fsk_demod_stream's hard bits, rows of Fb channel bytes are
 * de-scrambled, the CRC of the first P bytes is computed and compared with the received one, and
 * the payload is written out with a record and a status (check).  One handle, two directions.
 * Frames are independent; nothing is carried.  Integer arithmetic only.
 * The law is csrc/crc_law.h, one header the kernels and the host plan both compile.
 * CRC: width w in {8, 16, 24, 32}; poly below 2^w with the top term implicit and bit 0 set; init and
 * xorout below 2^w; reflect 0 or 1, applying to the input bytes and to the final register alike
 * (models with refin != refout are not offered).  Bit by bit: r = init; for each byte b of the
 * payload in order (bit-reversed when reflect) r ^= b << (w-8), then eight times
 * r = (r & top) ? ((r << 1) ^ poly) & mask : (r << 1) & mask; at the end r is bit-reversed over w
 * bits when reflect, then XORed with xorout.  The w/8 CRC bytes follow the payload most significant
 * byte first when reflect = 0 and least significant first when reflect = 1: the order in which the
 * model's residue property holds.  CRC-32/ISO-HDLC (zlib's) is (32, 0x04C11DB7, 0xFFFFFFFF, 1,
 * 0xFFFFFFFF); CRC-16/XMODEM is (16, 0x1021, 0, 0, 0).  The serial statement is the law; the host
 * plan runs it a byte at a time through a table, the kernels spread a frame over lanes.
 * Scrambler (additive, frame-synchronous: it restarts at every frame): degree m in [2, 32]; taps
 * below 2^m with bit 0 set; seed in [1, 2^m).  a[i] = bit i of seed for i < m; a[n+m] = the XOR over
 * the set bits i of taps of a[n+i]; bytes MSB first, a[8j] is bit 7 of byte j.  (8, 0xA9, 0xFF) is
 * the CCSDS randomiser, ff 48 0e c0 9a ...; (7, 0x09, 0x7F) gives from bit 7 on the IEEE 802.11
 * sequence 00001110 11110010 ...  m = 0: no scrambler.  w = 0: no CRC, a scrambler-only handle with
 * Fb = P, status 0 or 2 and record (0, 0).  Both zero is refused.
 * Frame: P in [1, 2^20], fixed at create.  Transmit: frame = (payload || crc bytes) XOR pn[0 .. Fb).
 * Receive, per frame b: r = channel XOR pn; P bytes r[0 .. P) at d_out + b*out_stride; two uint32
 * words at d_rec + 2b -- the CRC computed over r[0 .. P), and the CRC received in r[P .. Fb); an
 * int32 status at d_status + b:
 *   0  equal
 *   1  different; the payload is still written, as received
 *   2  d_status_in is given and its word for this frame is not 0: no input is read, the bytes are
 *      0, the record (0, 0) -- the convention of sfe_dsp_reed_*
 * Promised about bytes: the same call gives the same bytes on every run; a frame's output depends
 * on its bytes and the handle only -- never on b, n_frames, addresses, alignment or strides; the
 * device's bytes, record and status EQUAL sfe_dsp_crc_plan's for every input, none excluded;
 * nothing outside the slots named is written, to the byte.  Payloads and frames need no alignment;
 * records and statuses 4 bytes.
 * Out of scope: per-frame lengths or seeds, multiplicative (self-synchronising) scramblers, other
 * widths and refin != refout, CRCs over bits rather than bytes, compaction of the good frames,
 * differential encoding, in-place operation.
 * A bad argument is SFE_EINVAL on any machine, with a message that starts with "crc: ". */
typedef void *sfe_crc_t; /* opaque: one model, one sequence, one payload length; it owns its constants and its sequence on the device and nothing in it changes after create */
/* Host-only: n bytes of the scrambler's sequence by the law above into out.  m = 0 is refused here.
 * Also what makes sfe_dsp_reed_*'s `whiten`. */
int sfe_dsp_crc_pn_bytes(int m, uint32_t taps, uint32_t seed, size_t n, uint8_t *out);
/* Host-only (no GPU): validates what create validates and reports Fb (the pointer may be NULL).
 * With in != NULL -- host memory laid out as d_payload of append_stream (check = 0) or as d_frame
 * of check_stream (check = 1) -- it runs n_frames frames by the law above into out (frame b at
 * out + b*out_stride), record [n_frames][2] and status [n_frames]; each of the three may be NULL.
 * status_in [n_frames] or NULL; with check = 0 status_in, record and status are ignored.  The
 * reference of the device's bytes.  Short strides are SFE_ERANGE. */
int sfe_dsp_crc_plan(int width, uint32_t poly, uint32_t init, int reflect, uint32_t xorout,
                     int pn_m, uint32_t pn_taps, uint32_t pn_seed, int payload_bytes, int check,
                     const uint8_t *in, size_t in_stride, const int *status_in, size_t n_frames,
                     uint8_t *out, size_t out_stride, uint32_t *record, int *status,
                     int *frame_bytes);
/* Arguments are checked before the device is touched: SFE_EINVAL for a bad one on any machine,
 * SFE_ENODEV without a GPU.  The constants of the kernels and the sequence are made here. */
int sfe_dsp_crc_create(int width, uint32_t poly, uint32_t init, int reflect, uint32_t xorout,
                       int pn_m, uint32_t pn_taps, uint32_t pn_seed, int payload_bytes, int device,
                       sfe_crc_t *out);
/* n_frames frames each way.  d_status_in may be NULL; in check_stream d_out, d_rec and d_status
 * may each be NULL (a verify-only call), all three NULL is SFE_EINVAL.  *n_out = n_frames;
 * n_frames = 0 is a no-op.  A stride below the bytes a frame reads or writes (P, Fb) is SFE_ERANGE;
 * a null d_payload or d_frame, a misaligned record or status pointer, n_frames >= 2^31, a stride
 * that takes a buffer's byte range to 2^62, and any output byte range that overlaps an input's or
 * another output's are SFE_EINVAL, each with a message that starts with "crc_append_stream: " or
 * "crc_check_stream: "; nothing is launched on a refusal.  Asynchronous on `stream`; one kernel
 * launch and nothing else: allocates nothing, does not synchronise the host, carries no state
 * (there is no reset, and a handle has no setter), so a call on a stream under graph capture IS
 * supported.  Every loop of the kernels runs a number of times fixed by P and w. */
int sfe_dsp_crc_append_stream(sfe_crc_t h, const void *d_payload, size_t in_stride,
                              size_t n_frames, void *d_frame, size_t out_stride, size_t *n_out,
                              sfe_stream_t stream);
int sfe_dsp_crc_check_stream(sfe_crc_t h, const void *d_frame, size_t in_stride,
                             const void *d_status_in, size_t n_frames, void *d_out,
                             size_t out_stride, void *d_rec, void *d_status, size_t *n_out,
                             sfe_stream_t stream);
int sfe_dsp_crc_destroy(sfe_crc_t h);

#ifdef __cplusplus
}
#endif
#endif /* SFE_DSP_H_ */
