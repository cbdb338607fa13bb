"""Python face of libsfe_dsp.so.

Two layers, both thin:
  * `blkconv`, `resample`, `decimate` -- the reference's SWIG projection
    (libdsp/test/pydsp.i:16-22): same class names, same constructor arguments, and
    `process(in_array, out_len, rate) -> (n_out, out_array)` for the resamplers, so the
    reference's driver scripts (libdsp/test/test_decimate.py:22-25) read the same.
  * `Fir`, `Rs`, `DeviceArray` -- the device-resident bulk path used by bench.py and the
    parity tests (sfe_dsp_*_process_stream); `Chan`, the polyphase channelizer (sfe_dsp_chan_*); `Combiner`, its
    transpose, the synthesis filter bank (sfe_dsp_combine_*); `Psd`, the streaming Welch spectrum estimator (sfe_dsp_psd_*);
    `Corr`, the streaming preamble correlator bank (sfe_dsp_corr_*); `Iir`, the streaming biquad-cascade IIR filter
    (sfe_dsp_iir_*); `Beam`, the multi-stream beamformer / stream-mixing bank (sfe_dsp_beam_*); `Cov`, the streaming
    spatial covariance estimator (sfe_dsp_cov_*); `Mod`, the burst modulator (sfe_dsp_mod_*); `Polar`, the FM, phase and
    envelope detector (sfe_dsp_polar_*); `Occ`, the spectrum occupancy detector over a Psd's rows (sfe_dsp_occ_*);
    `Reed`, the interleaved Reed-Solomon outer code behind a Vit and in front of a Mod (sfe_dsp_reed_*); `Crc`, the frame
    check outside it, CRC and scrambler (sfe_dsp_crc_*); `Ofdm`, the OFDM burst
    receiver behind a Corr (sfe_dsp_ofdm_*); `OfdmMod`, its transmit side, the OFDM burst modulator (sfe_dsp_ofdmmod_*).

Everything computes on the GPU through the C ABI; numpy is only the host container.
"""
import ctypes as C

import numpy as np

from . import lib as _l
from .lib import SfeError, check  # noqa: F401


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def device_count():
    n = C.c_int(0)
    check(_l.load().sfe_dsp_device_count(C.byref(n)))
    return n.value


def sync(stream=None):
    check(_l.load().sfe_dsp_sync(stream))


class DeviceArray:
    """A flat float32 device buffer (sfe_dsp_malloc / sfe_dsp_free)."""

    def __init__(self, n_floats):
        self._L = _l.load()
        self.n = int(n_floats)
        p = C.c_void_p()
        check(self._L.sfe_dsp_malloc(C.byref(p), self.n * 4))
        self.ptr = p.value

    @classmethod
    def from_numpy(cls, a, stream=None):
        a = _f32(a).ravel()
        d = cls(a.size)
        check(d._L.sfe_dsp_memcpy_h2d(d.ptr, a.ctypes.data, a.nbytes, stream))
        check(d._L.sfe_dsp_sync(stream))
        return d

    @classmethod
    def from_bytes(cls, b, stream=None):
        """Device copy of a uint8 array (the u8 wire format), padded to whole floats."""
        b = np.ascontiguousarray(b, dtype=np.uint8).ravel()
        d = cls((b.size + 3) // 4 + 4)
        check(d._L.sfe_dsp_memcpy_h2d(d.ptr, b.ctypes.data, b.nbytes, stream))
        check(d._L.sfe_dsp_sync(stream))
        return d

    def to_numpy(self, n_floats=None, offset=0, stream=None):
        n = self.n - offset if n_floats is None else int(n_floats)
        out = np.empty(n, dtype=np.float32)
        check(self._L.sfe_dsp_memcpy_d2h(out.ctypes.data, self.ptr + 4 * int(offset), out.nbytes, stream))
        check(self._L.sfe_dsp_sync(stream))
        return out

    def fill_synth(self, seed, channel=0, first=0, n_floats=None, offset=0, stream=None):
        n = self.n - offset if n_floats is None else int(n_floats)
        check(self._L.sfe_dsp_synth_fill(self.ptr + 4 * int(offset), n, seed, channel, first, stream))

    def zero(self, stream=None):
        check(self._L.sfe_dsp_memset(self.ptr, 0, self.n * 4, stream))

    def free(self):
        if getattr(self, "ptr", None):
            self._L.sfe_dsp_free(self.ptr)
            self.ptr = None

    __del__ = free


class Timer:
    """HIP events on the stream the kernels are launched on (bench.py roofline leg)."""

    def __init__(self):
        self._L = _l.load()
        p = C.c_void_p()
        check(self._L.sfe_dsp_timer_create(C.byref(p)))
        self._h = p.value

    def start(self, stream=None):
        check(self._L.sfe_dsp_timer_start(self._h, stream))

    def stop(self, stream=None):
        check(self._L.sfe_dsp_timer_stop(self._h, stream))

    def elapsed_ms(self):
        ms = C.c_float(0)
        check(self._L.sfe_dsp_timer_elapsed_ms(self._h, C.byref(ms)))
        return ms.value

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.sfe_dsp_timer_destroy(self._h)
            self._h = None


class Fir:
    """One FIR stream set (sfe_dsp_fir_*): taps real (n,) or complex (n,) complex64."""

    def __init__(self, taps, data_complex=True, n_channels=1, block_hint=0, device=0, algo=_l.FIR_ALGO_AUTO,
                 per_channel=False):
        self._L = _l.load()
        taps = np.asarray(taps)
        self.taps_complex = bool(np.iscomplexobj(taps))
        if per_channel:
            # taps: (n_channels, n_taps), one filter per channel (sfe_dsp_fir_create_per_channel); cf32 streams
            assert taps.ndim == 2
            n_channels, n_taps = taps.shape
            t = (np.ascontiguousarray(taps.astype(np.complex64)).view(np.float32) if self.taps_complex
                 else _f32(taps)).reshape(-1)
            self.n_taps, self.data_complex, self.out_complex, self.n_channels = n_taps, True, True, n_channels
            h = C.c_void_p()
            check(self._L.sfe_dsp_fir_create_per_channel(t.ctypes.data, n_taps, int(self.taps_complex), n_channels,
                                                         device, C.byref(h)))
            self._h = h.value
            return
        if self.taps_complex:
            t = np.ascontiguousarray(taps.astype(np.complex64)).view(np.float32)
            n_taps = t.size // 2
        else:
            t = _f32(taps)
            n_taps = t.size
        self.n_taps = n_taps
        self.data_complex = bool(data_complex)
        self.out_complex = self.data_complex or self.taps_complex
        self.n_channels = n_channels
        h = C.c_void_p()
        check(self._L.sfe_dsp_fir_create(t.ctypes.data, n_taps, int(self.taps_complex), int(self.data_complex),
                                         n_channels, block_hint, device, C.byref(h)))
        self._h = h.value
        if algo != _l.FIR_ALGO_AUTO:
            self.set_algo(algo)

    def set_algo(self, algo):
        check(self._L.sfe_dsp_fir_set_algo(self._h, algo))

    def set_variant(self, variant):
        """lib.FIR_VARIANT_*: fix the cf32 kernel's data-movement variant (AUTO: what calibrate() chose for the
        shape, register loads where nothing was calibrated)."""
        check(self._L.sfe_dsp_fir_set_variant(self._h, int(variant)))

    def get_variant(self):
        """(variant of the last bulk call, calibrations made by this handle, [median ms per variant])."""
        v, k = C.c_int(-1), C.c_int(0)
        ms = (C.c_float * 3)()
        check(self._L.sfe_dsp_fir_get_variant(self._h, C.byref(v), C.byref(k), ms))
        return v.value, k.value, [float(m) for m in ms]

    def calibrate(self, d_in, d_out, n, in_stride=None, out_stride=None, stream=None):
        """sfe_dsp_fir_calibrate: time the kernel's variants over these buffers (synchronous; the stream
        does not advance) and remember the choice for this shape; returns the chosen variant."""
        pi = d_in.ptr if isinstance(d_in, DeviceArray) else int(d_in)
        po = d_out.ptr if isinstance(d_out, DeviceArray) else int(d_out)
        v = C.c_int(0)
        check(self._L.sfe_dsp_fir_calibrate(self._h, pi, po, n, n if in_stride is None else in_stride,
                                            n if out_stride is None else out_stride, stream, C.byref(v)))
        return v.value

    def set_zero_copy_max(self, max_samples):
        check(self._L.sfe_dsp_fir_set_zero_copy_max(self._h, int(max_samples)))

    def set_input_format(self, fmt):
        """lib.FMT_U8: process_stream reads u8 offset-binary samples (fused RX converter)."""
        check(self._L.sfe_dsp_fir_set_input_format(self._h, fmt))

    def set_output_format(self, fmt):
        """lib.FMT_TX10: process_stream writes 10-bit packed bytes (fused TX converter, real streams)."""
        check(self._L.sfe_dsp_fir_set_output_format(self._h, fmt))

    def reset(self):
        check(self._L.sfe_dsp_fir_reset(self._h))

    def load_history(self, d_prev, n_prev, stride=None, stream=None):
        """Carried state from the n_prev samples that precede the next call's input (one stream cut
        into spans): d_prev a DeviceArray or raw device pointer, float32 elements."""
        p = d_prev.ptr if isinstance(d_prev, DeviceArray) else int(d_prev or 0)
        check(self._L.sfe_dsp_fir_load_history(self._h, p, n_prev, n_prev if stride is None else stride, stream))

    def process_stream(self, d_in, d_out, n, in_stride=None, out_stride=None, stream=None):
        """d_in/d_out: DeviceArray or raw device pointers; n samples per channel."""
        pi = d_in.ptr if isinstance(d_in, DeviceArray) else int(d_in)
        po = d_out.ptr if isinstance(d_out, DeviceArray) else int(d_out)
        check(self._L.sfe_dsp_fir_process_stream(self._h, pi, po, n, n if in_stride is None else in_stride,
                                                 n if out_stride is None else out_stride, stream))

    def filter(self, x):
        """Host convenience: x is (n_channels, n*) float32 with interleaved I/Q when complex."""
        x = _f32(x).reshape(self.n_channels, -1)
        n = x.shape[1] // (2 if self.data_complex else 1)
        d_in = DeviceArray.from_numpy(x)
        d_out = DeviceArray(self.n_channels * n * (2 if self.out_complex else 1))
        self.process_stream(d_in, d_out, n)
        y = d_out.to_numpy().reshape(self.n_channels, -1)
        d_in.free()
        d_out.free()
        return y

    def host_buffer(self):
        p = C.POINTER(C.c_float)()
        blk = C.c_int(0)
        check(self._L.sfe_dsp_fir_host_buffer(self._h, C.byref(p), C.byref(blk)))
        width = 2 if self.out_complex else 1
        return np.ctypeslib.as_array(p, shape=(blk.value * width,)), blk.value

    def process_block(self):
        check(self._L.sfe_dsp_fir_process_block(self._h))

    def close(self):
        """sfe_dsp_fir_destroy.  A handle a pipe still borrows is NOT destroyed (SFE_ESTATE): it is kept,
        with a warning, rather than dropped on the floor with its GPU buffers."""
        if getattr(self, "_h", None):
            rc = self._L.sfe_dsp_fir_destroy(self._h)
            if rc == _l.SFE_ESTATE:
                import warnings
                warnings.warn("Fir.close: a pipe still borrows this handle (sfe_dsp_pipe_destroy first); handle kept",
                              ResourceWarning, stacklevel=2)
                return
            self._h = None

    __del__ = close


class _Group:
    """Channel blocks of one multi-channel job on several devices of THIS process (sfe_dsp_*_group_*;
    the partition of shard.channel_block made inside the library)."""
    _prefix = None

    def _fn(self, name):
        return getattr(self._L, "sfe_dsp_%s_group_%s" % (self._prefix, name))

    def shards(self):
        """[(device, first_channel, n_channels, handle, stream), ...]"""
        n = C.c_int(0)
        check(self._fn("shards")(self._g, C.byref(n)))
        out = []
        for k in range(n.value):
            d, f, c, h, s = C.c_int(0), C.c_int(0), C.c_int(0), C.c_void_p(), C.c_void_p()
            check(self._fn("shard")(self._g, k, C.byref(d), C.byref(f), C.byref(c), C.byref(h), C.byref(s)))
            out.append((d.value, f.value, c.value, h.value, s.value))
        return out

    @staticmethod
    def _ptrs(arrs):
        return (C.c_void_p * len(arrs))(*[a.ptr if isinstance(a, DeviceArray) else int(a) for a in arrs])

    def sync(self):
        check(self._fn("sync")(self._g))

    def reset(self):
        check(self._fn("reset")(self._g))

    def close(self):
        if getattr(self, "_g", None):
            self._fn("destroy")(self._g)
            self._g = None

    __del__ = close


class FirGroup(_Group):
    _prefix = "fir"

    def __init__(self, taps, n_channels, devices, data_complex=True, per_channel=False):
        self._L = _l.load()
        taps = np.asarray(taps)
        ctaps = bool(np.iscomplexobj(taps))
        t = (np.ascontiguousarray(taps.astype(np.complex64)).view(np.float32) if ctaps else _f32(taps)).reshape(-1)
        n_taps = taps.shape[-1]
        dv = (C.c_int * len(devices))(*[int(d) for d in devices])
        g = C.c_void_p()
        check(self._L.sfe_dsp_fir_group_create(t.ctypes.data, n_taps, int(ctaps), int(data_complex), int(per_channel),
                                               n_channels, dv, len(devices), C.byref(g)))
        self._g = g.value

    def process_stream(self, d_in, d_out, n, in_stride=None, out_stride=None):
        """d_in / d_out: one DeviceArray (or raw device pointer) per shard; asynchronous on the shards' streams."""
        check(self._L.sfe_dsp_fir_group_process_stream(self._g, self._ptrs(d_in), self._ptrs(d_out), n,
                                                       n if in_stride is None else in_stride,
                                                       n if out_stride is None else out_stride))


class RsGroup(_Group):
    _prefix = "rs"

    def __init__(self, taps, upsample, blksize, n_channels, devices, mode=_l.RS_RESAMPLE, data_complex=True):
        self._L = _l.load()
        t = _f32(taps)
        dv = (C.c_int * len(devices))(*[int(d) for d in devices])
        g = C.c_void_p()
        check(self._L.sfe_dsp_rs_group_create(t.ctypes.data, t.size, upsample, blksize, int(data_complex), n_channels,
                                              dv, len(devices), mode, C.byref(g)))
        self._g = g.value

    def process_stream(self, d_in, n_in, d_out, out_cap, rate, in_stride=None, out_stride=None):
        k = C.c_size_t(0)
        check(self._L.sfe_dsp_rs_group_process_stream(self._g, self._ptrs(d_in), n_in, n_in if in_stride is None else in_stride,
                                                      self._ptrs(d_out), out_cap, out_cap if out_stride is None else out_stride,
                                                      rate, C.byref(k)))
        return k.value


class Rs:
    """One resample/decimate stream set (sfe_dsp_rs_*)."""

    def __init__(self, taps, upsample, blksize, mode=_l.RS_RESAMPLE, data_complex=False, n_channels=1, device=0,
                 algo=_l.RS_ALGO_AUTO):
        self._L = _l.load()
        t = _f32(taps)
        self.data_complex = bool(data_complex)
        self.n_channels = n_channels
        self.upsample = upsample
        self.blksize = blksize
        h = C.c_void_p()
        check(self._L.sfe_dsp_rs_create(t.ctypes.data, t.size, upsample, blksize, int(self.data_complex),
                                        n_channels, device, mode, C.byref(h)))
        self._h = h.value
        if algo != _l.RS_ALGO_AUTO:
            self.set_algo(algo)

    def set_exact(self, exact=True):
        check(self._L.sfe_dsp_rs_set_exact(self._h, int(bool(exact))))

    def set_algo(self, algo):
        """lib.RS_ALGO_AUTO / DIRECT / FFT / MFMA: the kernel of the integer-step bulk path."""
        check(self._L.sfe_dsp_rs_set_algo(self._h, algo))

    def set_input_format(self, fmt):
        check(self._L.sfe_dsp_rs_set_input_format(self._h, fmt))

    def reset(self):
        check(self._L.sfe_dsp_rs_reset(self._h))

    def load_history(self, d_prev, n_prev, stride=None, stream=None):
        p = d_prev.ptr if isinstance(d_prev, DeviceArray) else int(d_prev or 0)
        check(self._L.sfe_dsp_rs_load_history(self._h, p, n_prev, n_prev if stride is None else stride, stream))

    def seek(self, first_sample, rate):
        """Time state of a reference object that has consumed `first_sample` samples (integer-valued
        steps only; raises SfeError(SFE_ESTATE) otherwise)."""
        check(self._L.sfe_dsp_rs_seek(self._h, int(first_sample), float(rate)))

    def get_state(self):
        st = _l.TimeState()
        check(self._L.sfe_dsp_rs_get_state(self._h, C.byref(st)))
        return st

    def set_state(self, st):
        check(self._L.sfe_dsp_rs_set_state(self._h, C.byref(st)))

    def process(self, x, out_len, rate):
        """Host-pointer call == {resample,decimate}::process; returns (n_out, out_array)."""
        x = _f32(x)
        w = 2 if self.data_complex else 1
        n_in = x.size // w
        out = np.zeros((out_len + 1) * w, dtype=np.float32)
        n = C.c_int(0)
        check(self._L.sfe_dsp_rs_process(self._h, x.ctypes.data, n_in, out.ctypes.data, out_len, rate, C.byref(n)))
        return n.value, out[: out_len * w]

    def process_stream(self, d_in, n_in, d_out, out_cap, rate, in_stride=None, out_stride=None, stream=None):
        pi = d_in.ptr if isinstance(d_in, DeviceArray) else int(d_in)
        po = d_out.ptr if isinstance(d_out, DeviceArray) else int(d_out)
        n = C.c_size_t(0)
        check(self._L.sfe_dsp_rs_process_stream(self._h, pi, n_in, n_in if in_stride is None else in_stride, po,
                                                out_cap, out_cap if out_stride is None else out_stride, rate,
                                                C.byref(n), stream))
        return n.value

    def resample_array(self, x, rate, chunk=None):
        """Host convenience for tests: feed x (n_channels, n*) through process_stream in
        `chunk`-sample calls (default: all at once); returns (n_channels, n_out*)."""
        x = _f32(x).reshape(self.n_channels, -1)
        w = 2 if self.data_complex else 1
        n = x.shape[1] // w
        chunk = chunk or n
        d_in = DeviceArray(self.n_channels * chunk * w)
        cap = int(np.ceil(chunk / min(rate, 1e9))) + 4
        d_out = DeviceArray(self.n_channels * cap * w)
        outs = []
        for off in range(0, n, chunk):
            m = min(chunk, n - off)
            seg = np.ascontiguousarray(x[:, off * w:(off + m) * w])
            check(self._L.sfe_dsp_memcpy_h2d(d_in.ptr, seg.ctypes.data, seg.nbytes, None))
            k = self.process_stream(d_in, m, d_out, cap, rate, in_stride=m, out_stride=cap)
            y = d_out.to_numpy(self.n_channels * cap * w).reshape(self.n_channels, cap * w)[:, : k * w]
            outs.append(y.copy())
        d_in.free()
        d_out.free()
        return np.concatenate(outs, axis=1) if outs else np.zeros((self.n_channels, 0), np.float32)

    def close(self):
        """sfe_dsp_rs_destroy; a handle a pipe still borrows is kept, with a warning (see Fir.close)."""
        if getattr(self, "_h", None):
            rc = self._L.sfe_dsp_rs_destroy(self._h)
            if rc == _l.SFE_ESTATE:
                import warnings
                warnings.warn("Rs.close: a pipe still borrows this handle (sfe_dsp_pipe_destroy first); handle kept",
                              ResourceWarning, stacklevel=2)
                return
            self._h = None

    __del__ = close


class _Block:
    """What the wrappers of the streaming blocks share: the handle behind `_h`, made by sfe_dsp_<_prefix>_create and
    destroyed by close(), the block's reset, and the pointer and upload plumbing of their calls."""
    _prefix = None              # the block's functions are sfe_dsp_<_prefix>_*

    def _fn(self, name):
        return getattr(self._L, "sfe_dsp_%s_%s" % (self._prefix, name))

    def _create(self, *args):
        self._L = _l.load()
        h = C.c_void_p()
        check(self._fn("create")(*args, C.byref(h)))
        self._h = h.value

    @staticmethod
    def _ptr(d):
        return d.ptr if isinstance(d, DeviceArray) else (None if d is None else int(d))

    def _set_input_format(self, fmt):
        check(self._fn("set_input_format")(self._h, fmt))
        self.in_u8 = fmt == _l.FMT_U8

    def _process_stream(self, d_in, n_in, in_stride, d_out, out_stride, stream):
        """The call most blocks share; in_stride None: n_in.  Returns what the library counted."""
        k = C.c_size_t(0)
        check(self._fn("process_stream")(self._h, self._ptr(d_in), int(n_in), int(n_in) if in_stride is None else int(in_stride),
                                         self._ptr(d_out), int(out_stride), C.byref(k), stream))
        return k.value

    def _upload_input(self, x, granule=1):
        """x as (n_streams, n) samples in the handle's input format -- (I,Q) bytes with FMT_U8, complex64, or float32 on a
        real handle -- each row padded with zero samples to a multiple of `granule`; returns (its DeviceArray, n)."""
        if self.in_u8:
            a, w, zero = np.ascontiguousarray(x, dtype=np.uint8).reshape(self.n_streams, -1), 2, 128   # byte 128 converts to 0.0
        elif getattr(self, "data_complex", True):     # the blocks without a real form have no such attribute
            a, w, zero = np.ascontiguousarray(x, dtype=np.complex64).reshape(self.n_streams, -1).view(np.float32), 2, 0
        else:
            a, w, zero = np.ascontiguousarray(x, dtype=np.float32).reshape(self.n_streams, -1), 1, 0
        n = a.shape[1] // w
        npad = -(-n // granule) * granule
        if npad != n:
            a = np.concatenate([a[:, :w * n], np.full((self.n_streams, w * (npad - n)), zero, a.dtype)], axis=1)
        return (DeviceArray.from_bytes(a) if self.in_u8 else DeviceArray.from_numpy(a)), n

    def reset(self):
        check(self._fn("reset")(self._h))

    def close(self):
        if getattr(self, "_h", None):
            self._fn("destroy")(self._h)
            self._h = None

    __del__ = close


def chan_plan(n_taps, n_chans, decim):
    """sfe_dsp_chan_plan (host only, no GPU): (taps per branch P, samples of history carried per stream)."""
    P, H = C.c_int(0), C.c_int(0)
    check(_l.load().sfe_dsp_chan_plan(int(n_taps), int(n_chans), int(decim), C.byref(P), C.byref(H)))
    return P.value, H.value


class Chan(_Block):
    """Polyphase filter-bank channelizer (sfe_dsp_chan_*): n_chans = M sub-bands of n_streams complex streams, one
    output every `decim` (M or M/2) input samples per channel; real prototype taps."""
    _prefix = "chan"

    def __init__(self, taps, n_chans, decim, n_streams=1, device=0):
        t = _f32(taps)
        self.n_chans, self.decim, self.n_streams = int(n_chans), int(decim), int(n_streams)
        self.in_u8 = False
        self._create(t.ctypes.data, t.size, self.n_chans, self.decim, self.n_streams, device)

    def set_input_format(self, fmt):
        """lib.FMT_F32 (cf32) or lib.FMT_U8 ((I,Q) byte pairs, converted on load)."""
        self._set_input_format(fmt)

    def process_stream(self, d_in, n_in, d_out, in_stride=None, out_stride=None, stream=None):
        """d_in / d_out: DeviceArray or raw device pointers; n_in samples per stream (a multiple of decim).  Channel k
        of stream s goes to d_out + (s*M + k)*out_stride cf32 samples.  Returns n_out = n_in / decim."""
        return self._process_stream(d_in, n_in, in_stride, d_out, int(n_in) // self.decim if out_stride is None else out_stride, stream)

    def channelize(self, x):
        """Host convenience, computed on the GPU: x is (n_streams, n) complex -- or, with FMT_U8, (n_streams, 2n)
        uint8 (I,Q) pairs -- (1-D for one stream); returns (n_streams, M, n // decim) complex64."""
        d_in, n = self._upload_input(x)
        n_out = n // self.decim
        d_out = DeviceArray(max(1, self.n_streams * self.n_chans * n_out) * 2)
        try:
            k = self.process_stream(d_in, n, d_out)
            y = d_out.to_numpy(self.n_streams * self.n_chans * k * 2)
        finally:
            d_in.free()
            d_out.free()
        return y.view(np.complex64).reshape(self.n_streams, self.n_chans, k)


def combine_plan(n_taps, n_chans, interp):
    """sfe_dsp_combine_plan (host only, no GPU): (taps per output phase P, instants of history carried per stream)."""
    P, H = C.c_int(0), C.c_int(0)
    check(_l.load().sfe_dsp_combine_plan(int(n_taps), int(n_chans), int(interp), C.byref(P), C.byref(H)))
    return P.value, H.value


class Combiner(_Block):
    """Polyphase synthesis filter bank (sfe_dsp_combine_*): n_chans = M baseband channels of n_streams streams, each
    interpolated by `interp` (M or M/2), shifted up to its sub-band and summed; real prototype taps."""
    _prefix = "combine"

    def __init__(self, taps, n_chans, interp, n_streams=1, device=0):
        t = _f32(taps)
        self.n_chans, self.interp, self.n_streams = int(n_chans), int(interp), int(n_streams)
        self.out_tx10 = False
        self._create(t.ctypes.data, t.size, self.n_chans, self.interp, self.n_streams, device)

    def set_output_format(self, fmt):
        """lib.FMT_F32 (cf32) or lib.FMT_TX10 (the transmit wire format, 2 complex samples in 5 bytes)."""
        check(self._fn("set_output_format")(self._h, fmt))
        self.out_tx10 = fmt == _l.FMT_TX10

    def process_stream(self, d_in, n_in, d_out, in_stride=None, out_stride=None, stream=None):
        """d_in / d_out: DeviceArray or raw device pointers; n_in instants per channel.  Channel k of stream s is read at
        d_in + (s*M + k)*in_stride cf32 samples; stream s is written at d_out + s*out_stride samples (TX10: at
        s*(out_stride/2)*5 bytes).  Returns n_out = n_in * interp."""
        return self._process_stream(d_in, n_in, in_stride, d_out, int(n_in) * self.interp if out_stride is None else out_stride, stream)

    def combine(self, X):
        """Host convenience, computed on the GPU: X is (n_streams, M, n) complex ((M, n) for one stream); returns
        (n_streams, n * interp) complex64 -- or, with FMT_TX10, (n_streams, n * interp // 2 * 5) uint8."""
        z = np.ascontiguousarray(X, dtype=np.complex64).reshape(self.n_streams, self.n_chans, -1)
        n = z.shape[2]
        n_out = n * self.interp
        d_in = DeviceArray.from_numpy(z.view(np.float32))
        row_b = n_out // 2 * 5 if self.out_tx10 else 8 * n_out
        d_out = DeviceArray(max(1, (self.n_streams * row_b + 3) // 4))
        try:
            k = self.process_stream(d_in, n, d_out)
            y = d_out.to_numpy()
        finally:
            d_in.free()
            d_out.free()
        if self.out_tx10:
            return y.view(np.uint8)[: self.n_streams * (k // 2 * 5)].reshape(self.n_streams, -1)
        return y[: self.n_streams * 2 * k].view(np.complex64).reshape(self.n_streams, k)


def ddc_plan(n_taps, decim, freqs):
    """sfe_dsp_ddc_plan (host only, no GPU): (taps per branch P, samples of history carried per stream, the quantised
    32-bit NCO increments as a list of ints)."""
    f = np.ascontiguousarray(freqs, dtype=np.float64).ravel()
    P, H = C.c_int(0), C.c_int(0)
    inc = (C.c_uint32 * max(1, f.size))()
    check(_l.load().sfe_dsp_ddc_plan(int(n_taps), int(decim), int(f.size), f.ctypes.data_as(C.POINTER(C.c_double)), C.byref(P),
                                     C.byref(H), inc))
    return P.value, H.value, [int(v) for v in inc[:f.size]]


class Ddc(_Block):
    """Digital down-converter bank (sfe_dsp_ddc_*): len(freqs) = K tunings of n_streams streams, each shifted down by its
    frequency (cycles per sample, quantised to a 32-bit NCO increment), filtered by the real prototype `taps` and
    decimated by `decim`.  data_complex=False takes real float32 input; the output is always complex."""
    _prefix = "ddc"

    def __init__(self, taps, decim, freqs, data_complex=True, n_streams=1, device=0):
        t = _f32(taps)
        f = np.ascontiguousarray(freqs, dtype=np.float64).ravel()
        self.decim, self.n_tunings, self.n_streams = int(decim), int(f.size), int(n_streams)
        self.data_complex = bool(data_complex)
        self.in_u8 = False
        self._create(t.ctypes.data, t.size, self.decim, self.n_tunings, f.ctypes.data_as(C.POINTER(C.c_double)), int(self.data_complex),
                     self.n_streams, device)

    def set_input_format(self, fmt):
        """lib.FMT_F32 (cf32, or float32 for a real handle) or lib.FMT_U8 ((I,Q) byte pairs, converted on load)."""
        self._set_input_format(fmt)

    def set_freqs(self, freqs):
        """K new frequencies, used from the next call on (no phase continuity across the retune)."""
        f = np.ascontiguousarray(freqs, dtype=np.float64).ravel()
        if f.size != self.n_tunings:
            raise ValueError("set_freqs: %d frequencies for %d tunings" % (f.size, self.n_tunings))
        check(self._fn("set_freqs")(self._h, f.ctypes.data_as(C.POINTER(C.c_double))))

    def process_stream(self, d_in, n_in, d_out, in_stride=None, out_stride=None, stream=None):
        """d_in / d_out: DeviceArray or raw device pointers; n_in samples per stream (a multiple of decim).  Tuning k of
        stream s goes to d_out + (s*K + k)*out_stride cf32 samples.  Returns n_out = n_in / decim."""
        return self._process_stream(d_in, n_in, in_stride, d_out, int(n_in) // self.decim if out_stride is None else out_stride, stream)

    def downconvert(self, x):
        """Host convenience, computed on the GPU: x is (n_streams, n) complex -- real for a real handle, or, with FMT_U8,
        (n_streams, 2n) uint8 (I,Q) pairs -- (1-D for one stream); returns (n_streams, K, n // decim) complex64."""
        d_in, n = self._upload_input(x)
        n_out = n // self.decim
        d_out = DeviceArray(max(1, self.n_streams * self.n_tunings * n_out) * 2)
        try:
            k = self.process_stream(d_in, n, d_out)
            y = d_out.to_numpy(self.n_streams * self.n_tunings * k * 2)
        finally:
            d_in.free()
            d_out.free()
        return y.view(np.complex64).reshape(self.n_streams, self.n_tunings, k)


def psd_plan(n_fft, hop, n_avg):
    """sfe_dsp_psd_plan (host only, no GPU): (segments per chunk C of the summation order, samples of history carried
    per stream = n_fft - hop)."""
    c, h = C.c_int(0), C.c_int(0)
    check(_l.load().sfe_dsp_psd_plan(int(n_fft), int(hop), int(n_avg), C.byref(c), C.byref(h)))
    return c.value, h.value


class Psd(_Block):
    """Streaming Welch spectrum estimator (sfe_dsp_psd_*): scale times the sum of n_avg windowed periodograms of
    n_fft = len(window) samples, one every `hop` samples, of n_streams complex streams."""
    _prefix = "psd"

    def __init__(self, window, hop, n_avg, scale=1.0, n_streams=1, device=0):
        w = _f32(window).ravel()
        self.n_fft, self.hop, self.n_avg, self.n_streams = int(w.size), int(hop), int(n_avg), int(n_streams)
        self.in_u8 = False
        self._create(w.ctypes.data, self.n_fft, self.hop, self.n_avg, float(scale), self.n_streams, device)

    def set_input_format(self, fmt):
        """lib.FMT_F32 (cf32) or lib.FMT_U8 ((I,Q) byte pairs, converted on load)."""
        self._set_input_format(fmt)

    def process_stream(self, d_in, n_in, d_out, in_stride=None, out_stride=None, stream=None):
        """d_in / d_out: DeviceArray or raw device pointers; n_in samples per stream (a multiple of hop).  Row j of
        stream s that the call completes goes to d_out + s*out_stride + j*n_fft floats; out_stride defaults to the rows
        n_in samples can complete at the most.  Returns the number of rows written per stream."""
        most = -(-(int(n_in) // self.hop) // self.n_avg) * self.n_fft
        return self._process_stream(d_in, n_in, in_stride, d_out, most if out_stride is None else out_stride, stream)

    def spectrum(self, x):
        """Host convenience, computed on the GPU: x is (n_streams, n) complex64 -- or (n_streams, n, 2) uint8 (I,Q)
        pairs with FMT_U8 -- (one dimension less for one stream), n a multiple of hop; returns the rows the call
        completes, (n_streams, rows, n_fft) float32."""
        d_in, n = self._upload_input(x)
        stride = -(-(n // self.hop) // self.n_avg) * self.n_fft
        d_out = DeviceArray(max(1, self.n_streams * stride))
        try:
            k = self.process_stream(d_in, n, d_out, out_stride=stride)
            y = d_out.to_numpy(self.n_streams * stride).reshape(self.n_streams, -1, self.n_fft)[:, :k]
        finally:
            d_in.free()
            d_out.free()
        return np.ascontiguousarray(y)


def corr_plan(length, n_templates, block):
    """sfe_dsp_corr_plan (host only, no GPU): (transform advance V, samples of history carried per stream = 4096 - V)."""
    v, h = C.c_int(0), C.c_int(0)
    check(_l.load().sfe_dsp_corr_plan(int(length), int(n_templates), int(block), C.byref(v), C.byref(h)))
    return v.value, h.value


class Corr(_Block):
    """Streaming preamble correlator bank (sfe_dsp_corr_*): the squared normalised correlation of K complex templates
    (n_templates, len) against n_streams complex streams, reduced to (peak value, first peak offset) per block of
    `block` samples."""
    _prefix = "corr"

    def __init__(self, templates, block, min_energy=0.0, n_streams=1, device=0):
        t = np.atleast_2d(np.ascontiguousarray(templates, dtype=np.complex64))
        self.n_templates, self.len = int(t.shape[0]), int(t.shape[1])
        self.block, self.n_streams = int(block), int(n_streams)
        self.in_u8 = False
        self._create(t.view(np.float32).ctypes.data, self.len, self.n_templates, self.block, float(min_energy), self.n_streams, device)

    def set_input_format(self, fmt):
        """lib.FMT_F32 (cf32) or lib.FMT_U8 ((I,Q) byte pairs, converted on load)."""
        self._set_input_format(fmt)

    def process_stream(self, d_in, n_in, d_peak_val, d_peak_idx, d_metric=None, in_stride=None, peak_stride=None, metric_stride=None,
                       stream=None):
        """d_*: DeviceArray or raw device pointers; n_in samples per stream (a multiple of block).  Block j of template k
        of stream s goes to element (s*K + k)*peak_stride + j of d_peak_val (float32) and d_peak_idx (uint32), and with
        d_metric every m_k[i] to (s*K + k)*metric_stride + i; the strides default to n_in / block and n_in.  Returns the
        number of blocks."""
        ptr = self._ptr
        n_blocks = C.c_size_t(0)
        check(self._fn("process_stream")(self._h, ptr(d_in), int(n_in), int(n_in) if in_stride is None else int(in_stride),
                                         ptr(d_peak_val), ptr(d_peak_idx),
                                         int(n_in) // self.block if peak_stride is None else int(peak_stride), ptr(d_metric),
                                         int(n_in) if metric_stride is None else int(metric_stride), C.byref(n_blocks), stream))
        return n_blocks.value

    def search(self, x, dense=False):
        """Host convenience, computed on the GPU: x is (n_streams, n) complex64 -- or (n_streams, n, 2) uint8 (I,Q)
        pairs with FMT_U8 -- (one dimension less for one stream), n a multiple of block.  Returns (peak_val float32,
        peak_idx uint32), each (n_streams, K, n / block), and with dense=True also m, (n_streams, K, n) float32."""
        d_in, n = self._upload_input(x)
        rows, nb = self.n_streams * self.n_templates, n // self.block
        d_val, d_idx = DeviceArray(max(1, rows * nb)), DeviceArray(max(1, rows * nb))
        d_m = DeviceArray(max(1, rows * n)) if dense else None
        try:
            k = self.process_stream(d_in, n, d_val, d_idx, d_m)
            shape = (self.n_streams, self.n_templates, nb)
            out = (d_val.to_numpy(rows * nb).reshape(shape)[:, :, :k].copy(),
                   d_idx.to_numpy(rows * nb).view(np.uint32).reshape(shape)[:, :, :k].copy())
            if dense:
                out += (d_m.to_numpy(rows * n).reshape(self.n_streams, self.n_templates, n),)
        finally:
            d_in.free()
            d_val.free()
            d_idx.free()
            if d_m is not None:
                d_m.free()
        return out


def _sos(sos):
    a = np.atleast_2d(np.ascontiguousarray(sos, dtype=np.float64))
    if a.ndim != 2 or a.shape[1] != 6:
        raise ValueError("sos must be (n_sections, 6) rows of (b0, b1, b2, a0, a1, a2)")
    return np.ascontiguousarray(a)


def iir_plan(sos):
    """sfe_dsp_iir_plan (host only, no GPU): (block G, the granule of a call; float32 values of carried state per
    stream and component).  Raises SfeError on coefficients the filter refuses."""
    a = _sos(sos)
    g, st = C.c_int(0), C.c_int(0)
    check(_l.load().sfe_dsp_iir_plan(a.ctypes.data_as(C.POINTER(C.c_double)), int(a.shape[0]), C.byref(g), C.byref(st)))
    return g.value, st.value


class Iir(_Block):
    """Streaming biquad-cascade IIR filter (sfe_dsp_iir_*): `sos` is (n_sections, 6) float64 rows (b0, b1, b2, a0, a1, a2)
    (scipy's layout; synth.iir_* design some), run over n_streams complex (or, data_complex=False, real) streams."""
    _prefix = "iir"

    def __init__(self, sos, data_complex=True, n_streams=1, device=0):
        a = _sos(sos)
        self.n_sections, self.data_complex, self.n_streams = int(a.shape[0]), bool(data_complex), int(n_streams)
        self.in_u8 = False
        self._create(a.ctypes.data_as(C.POINTER(C.c_double)), self.n_sections, int(self.data_complex), self.n_streams, device)
        self.block = iir_plan(a)[0]

    def set_input_format(self, fmt):
        """lib.FMT_F32 (cf32, or float32 on a real handle) or lib.FMT_U8 ((I,Q) byte pairs, converted on load)."""
        self._set_input_format(fmt)

    def process_stream(self, d_in, n_in, d_out, in_stride=None, out_stride=None, stream=None):
        """d_in / d_out: DeviceArray or raw device pointers; n_in samples per stream (a multiple of self.block).  Stream s
        goes from d_in + s*in_stride to d_out + s*out_stride samples; both strides default to n_in.  Returns n_out = n_in."""
        return self._process_stream(d_in, n_in, in_stride, d_out, int(n_in) if out_stride is None else out_stride, stream)

    def filter(self, x):
        """Host convenience, computed on the GPU, continuing the handle's state: x is (n_streams, n) complex64 -- float32
        for a real handle, or (n_streams, n, 2) uint8 (I,Q) pairs with FMT_U8 -- (one dimension less for one stream).
        The tail is padded with zeros to a multiple of the block (the filter is causal: the padding changes no sample
        before it, but it does advance the state, so only the last piece of a stream may be ragged).  Returns x's
        samples filtered, (n_streams, n) (or (n,)) complex64 / float32."""
        G, S = self.block, self.n_streams
        one = S == 1 and np.ndim(x) <= 2 if self.in_u8 else np.ndim(x) == 1      # u8: (n, 2) or 2n bytes
        d_in, n = self._upload_input(x, G)
        npad = -(-n // G) * G
        w = 2 if self.data_complex else 1
        d_out = DeviceArray(max(1, S * npad * w))
        try:
            if npad:
                self.process_stream(d_in, npad, d_out)
            y = d_out.to_numpy(S * npad * w)
        finally:
            d_in.free()
            d_out.free()
        y = (y.view(np.complex64) if self.data_complex else y).reshape(S, npad)[:, :n]
        return np.ascontiguousarray(y[0] if one else y)


def _beam_weights(W, V):
    """(W as (M, B, S) complex64, V the same or None, their float pointers): (B, S) weights are one band."""
    W = np.asarray(W, dtype=np.complex64)
    W = np.ascontiguousarray(W[None] if W.ndim == 2 else W)
    if W.ndim != 3:
        raise ValueError("beam weights must be (n_beams, n_in) or (n_bands, n_beams, n_in) complex")
    if V is not None:
        V = np.ascontiguousarray(np.asarray(V, dtype=np.complex64).reshape(W.shape))
    fp = C.POINTER(C.c_float)
    return W, V, W.view(np.float32).ctypes.data_as(fp), (None if V is None else V.view(np.float32).ctypes.data_as(fp))


def beam_plan(W, V=None):
    """sfe_dsp_beam_plan (host only, no GPU): the real matrices R_k the kernel multiplies by, (M, 2B, 2S) float32.
    Raises SfeError on a shape or weights the block refuses."""
    W, V, pw, pv = _beam_weights(W, V)
    M, B, S = W.shape
    R = np.empty((M, 2 * B, 2 * S), dtype=np.float32)
    check(_l.load().sfe_dsp_beam_plan(S, B, M, pw, pv, R.ctypes.data_as(C.POINTER(C.c_float))))
    return R


class Beam(_Block):
    """Multi-stream beamformer / stream-mixing bank (sfe_dsp_beam_*): n_beams = B outputs out of n_in = S streams in each
    of n_bands = M bands, y_b = sum_s W[b][s] x_s + V[b][s] conj(x_s).  W (and V, optional) are (M, B, S) complex, or
    (B, S) for one band."""
    _prefix = "beam"

    def __init__(self, W, V=None, device=0):
        W, V, pw, pv = _beam_weights(W, V)
        self.n_bands, self.n_beams, self.n_in = (int(v) for v in W.shape)
        self.n_streams = self.n_in * self.n_bands           # rows of an input buffer
        self.in_u8 = False
        self._create(pw, pv, self.n_in, self.n_beams, self.n_bands, device)

    def set_input_format(self, fmt):
        """lib.FMT_F32 (cf32) or lib.FMT_U8 ((I,Q) byte pairs, converted on load)."""
        self._set_input_format(fmt)

    def set_weights(self, W, V=None):
        """New weights of the same shape, used from the next call on."""
        W, V, pw, pv = _beam_weights(W, V)
        if W.shape != (self.n_bands, self.n_beams, self.n_in):
            raise ValueError("set_weights: shape %s for a handle of %s" % (W.shape, (self.n_bands, self.n_beams, self.n_in)))
        check(self._fn("set_weights")(self._h, pw, pv))

    def process_stream(self, d_in, n_in, d_out, in_stride=None, out_stride=None, stream=None):
        """d_in / d_out: DeviceArray or raw device pointers; n_in >= 1 samples.  Band k of stream s is read at
        d_in + (s*M + k)*in_stride, band k of beam b written at d_out + (b*M + k)*out_stride cf32 samples; both strides
        default to n_in.  Returns n_out = n_in."""
        return self._process_stream(d_in, n_in, in_stride, d_out, int(n_in) if out_stride is None else out_stride, stream)

    def reset(self):
        raise AttributeError("Beam has no reset: it carries no state")

    def mix(self, x):
        """Host convenience, computed on the GPU: x is (S, M, n) complex64 ((S, n) for one band) -- or, with FMT_U8, uint8
        (I,Q) pairs with a last axis of 2n -- and the result (B, M, n) ((B, n)) complex64."""
        one = self.n_bands == 1 and np.ndim(x) == 2
        d_in, n = self._upload_input(x)
        d_out = DeviceArray(max(1, self.n_beams * self.n_bands * n) * 2)
        try:
            if n:
                self.process_stream(d_in, n, d_out)
            y = d_out.to_numpy(self.n_beams * self.n_bands * n * 2)
        finally:
            d_in.free()
            d_out.free()
        y = y.view(np.complex64).reshape(self.n_beams, self.n_bands, n)
        return np.ascontiguousarray(y[:, 0] if one else y)


def cov_plan(n_in, n_bands, n_avg):
    """sfe_dsp_cov_plan (host only, no GPU): (instants per chunk T, chunks per group C) of the summation order."""
    t, c = C.c_int(0), C.c_int(0)
    check(_l.load().sfe_dsp_cov_plan(int(n_in), int(n_bands), int(n_avg), C.byref(t), C.byref(c)))
    return t.value, c.value


class Cov(_Block):
    """Streaming spatial covariance estimator (sfe_dsp_cov_*): per band, scale times the sum over n_avg instants of
    u u^T, u the 2 n_in real floats of an instant of n_in = S complex streams; rows of (2S)^2 float32."""
    _prefix = "cov"

    def __init__(self, n_in, n_bands=1, n_avg=64, scale=1.0, device=0):
        self.n_in, self.n_bands, self.n_avg = int(n_in), int(n_bands), int(n_avg)
        self.n_streams = self.n_in * self.n_bands           # rows of an input buffer
        self.in_u8 = False
        self._create(self.n_in, self.n_bands, self.n_avg, float(scale), device)
        self.chunk = cov_plan(self.n_in, self.n_bands, self.n_avg)[0]

    def set_input_format(self, fmt):
        """lib.FMT_F32 (cf32) or lib.FMT_U8 ((I,Q) byte pairs, converted on load)."""
        self._set_input_format(fmt)

    def process_stream(self, d_in, n_in, d_out, in_stride=None, out_stride=None, stream=None):
        """d_in / d_out: DeviceArray or raw device pointers; n_in instants (a multiple of the chunk).  Band k of stream s
        is read at d_in + (s*M + k)*in_stride; row j of band k that the call completes goes to
        d_out + k*out_stride + j*(2S)^2 floats; out_stride defaults to the rows n_in instants can complete at the most.
        Returns the number of rows written per band."""
        most = -(-int(n_in) // self.n_avg) * 4 * self.n_in * self.n_in
        return self._process_stream(d_in, n_in, in_stride, d_out, most if out_stride is None else out_stride, stream)

    def gram(self, x):
        """Host convenience, computed on the GPU: x is (S, M, n) complex64 ((S, n) for one band) -- or, with FMT_U8, uint8
        (I,Q) pairs with a last axis of 2n -- n a multiple of the chunk; returns the rows the call completes,
        (M, rows, 2S, 2S) float32."""
        d_in, n = self._upload_input(x)
        n2 = 2 * self.n_in
        stride = -(-n // self.n_avg) * n2 * n2
        d_out = DeviceArray(max(1, self.n_bands * stride))
        try:
            k = self.process_stream(d_in, n, d_out, out_stride=stride)
            y = d_out.to_numpy(self.n_bands * stride).reshape(self.n_bands, -1, n2, n2)[:, :k]
        finally:
            d_in.free()
            d_out.free()
        return np.ascontiguousarray(y)


def _mvdr_steering(steering):
    """(steering as (M, B, S) complex64, its float pointer): (B, S) is one band."""
    a = np.asarray(steering, dtype=np.complex64)
    a = np.ascontiguousarray(a[None] if a.ndim == 2 else a)
    if a.ndim != 3:
        raise ValueError("steering must be (n_beams, n_in) or (n_bands, n_beams, n_in) complex")
    return a, a.view(np.float32).ctypes.data_as(C.POINTER(C.c_float))


def mvdr_plan(steering, G=None, widely_linear=False, load_rel=0.0, load_abs=0.0):
    """sfe_dsp_mvdr_plan (host only, no GPU): validates, and with G -- one row of Gram matrices, (M, 2S, 2S) or (2S, 2S)
    float32 -- solves it by the law in float64: returns (R (M, 2B, 2S) float32, power (M, B) float32, status (M,) int32),
    or None without G.  Raises SfeError on arguments the block refuses."""
    a, pa = _mvdr_steering(steering)
    M, B, S = a.shape
    fp, L = C.POINTER(C.c_float), _l.load()
    if G is None:
        check(L.sfe_dsp_mvdr_plan(S, B, M, pa, int(widely_linear), load_rel, load_abs, None, None, None, None))
        return None
    G = np.ascontiguousarray(np.asarray(G, dtype=np.float32).reshape(M, 2 * S, 2 * S))
    R, pw, st = np.empty((M, 2 * B, 2 * S), np.float32), np.empty((M, B), np.float32), np.empty(M, np.int32)
    check(L.sfe_dsp_mvdr_plan(S, B, M, pa, int(widely_linear), load_rel, load_abs, G.ctypes.data_as(fp), R.ctypes.data_as(fp),
                              pw.ctypes.data_as(fp), st.ctypes.data_as(C.POINTER(C.c_int))))
    return R, pw, st


class Mvdr(_Block):
    """Adaptive beamforming weight solver (sfe_dsp_mvdr_*): per row of Cov's output and band, the regularised MVDR weights
    of n_beams = B steering vectors over n_in = S streams as the real matrix Beam multiplies by, the per-beam output power
    (the Capon spectrum) and a status.  steering is (M, B, S) complex, or (B, S) for one band."""
    _prefix = "mvdr"

    def __init__(self, steering, widely_linear=False, load_rel=0.0, load_abs=0.0, device=0):
        a, pa = _mvdr_steering(steering)
        self.n_bands, self.n_beams, self.n_in = (int(v) for v in a.shape)
        self.widely_linear = bool(widely_linear)
        self._create(pa, self.n_in, self.n_beams, self.n_bands, int(self.widely_linear), load_rel, load_abs, device)

    def set_steering(self, steering):
        """New steering vectors of the same shape, used from the next call on."""
        a, pa = _mvdr_steering(steering)
        if a.shape != (self.n_bands, self.n_beams, self.n_in):
            raise ValueError("set_steering: shape %s for a handle of %s" % (a.shape, (self.n_bands, self.n_beams, self.n_in)))
        check(self._fn("set_steering")(self._h, pa))

    def set_loading(self, load_rel, load_abs=0.0):
        """A new diagonal loading, used from the next call on."""
        check(self._fn("set_loading")(self._h, load_rel, load_abs))

    def process_stream(self, d_gram, n_rows, d_R, d_power=None, d_status=None, in_stride=None, out_stride=None, power_stride=None,
                       status_stride=None, stream=None):
        """d_*: DeviceArray or raw device pointers.  Row j of band k is read at d_gram + k*in_stride + j*(2S)^2 floats
        (Cov's output; in_stride defaults to n_rows*(2S)^2); its matrix goes to d_R + j*out_stride + k*4BS, its powers to
        d_power + j*power_stride + k*B, its status (int32) to d_status + j*status_stride + k; the output strides default
        to one row's block.  Returns the number of rows solved."""
        M, B, n2 = self.n_bands, self.n_beams, 2 * self.n_in
        k = C.c_size_t(0)
        check(self._fn("process_stream")(
            self._h, self._ptr(d_gram), int(n_rows), int(n_rows) * n2 * n2 if in_stride is None else int(in_stride), self._ptr(d_R),
            M * 2 * B * n2 if out_stride is None else int(out_stride), self._ptr(d_power), M * B if power_stride is None else int(power_stride),
            self._ptr(d_status), M if status_stride is None else int(status_stride), C.byref(k), stream))
        return k.value

    def load_beam(self, beam, d_R, stream=None):
        """Hand one row's matrices (M, 2B, 2S), on the device, to a live Beam of the same shape: Beam calls enqueued later
        on `stream` use them.  No host copy and no wait."""
        check(self._L.sfe_dsp_mvdr_load_beam(getattr(beam, "_h", beam), self._ptr(d_R), stream))

    def reset(self):
        raise AttributeError("Mvdr has no reset: it carries no state")

    def solve(self, G):
        """Host convenience, computed on the GPU: G is (M, rows, 2S, 2S) float32 (Cov.gram's result; (M, 2S, 2S) and, for
        one band, (2S, 2S) are one row); returns (R (rows, M, 2B, 2S) float32, power (rows, M, B) float32,
        status (rows, M) int32)."""
        M, B, n2 = self.n_bands, self.n_beams, 2 * self.n_in
        G = np.ascontiguousarray(np.asarray(G, dtype=np.float32).reshape(M, -1, n2, n2))
        rows = G.shape[1]
        d_g, d_R = DeviceArray.from_numpy(G.ravel()), DeviceArray(max(1, rows * M * 2 * B * n2))
        d_p, d_s = DeviceArray(max(1, rows * M * B)), DeviceArray(max(1, rows * M))
        try:
            if rows:
                self.process_stream(d_g, rows, d_R, d_p, d_s)
            R = d_R.to_numpy(rows * M * 2 * B * n2).reshape(rows, M, 2 * B, n2)
            pw = d_p.to_numpy(rows * M * B).reshape(rows, M, B)
            st = d_s.to_numpy(rows * M).view(np.int32).reshape(rows, M)
        finally:
            for d in (d_g, d_R, d_p, d_s):
                d.free()
        return np.ascontiguousarray(R), np.ascontiguousarray(pw), np.ascontiguousarray(st)


def _eig_steering(steering, n_in, n_bands):
    """(steering as (M, B, S) complex64 -- None: (n_bands, 0, n_in) -- and its float pointer, null without beams)."""
    if steering is None:
        return np.zeros((int(n_bands), 0, int(n_in)), np.complex64), None
    return _mvdr_steering(steering)


def eig_plan(steering, G=None, widely_linear=False, signal_dim=0, n_vec=0, n_in=None, n_bands=1):
    """sfe_dsp_eig_plan (host only, no GPU): validates, and with G -- one row of Gram matrices, (M, 2S, 2S) or (2S, 2S)
    float32 -- decomposes it by the law in float64: returns (values (M, 2S), null (M, B), vectors (M, 2E, 2S), all
    float32, status (M,) int32), or None without G.  steering is (M, B, S) or (B, S) complex, or None (no beams: n_in and
    n_bands give the shape).  Raises SfeError on arguments the block refuses."""
    a, pa = _eig_steering(steering, n_in, n_bands)
    M, B, S = a.shape
    fp, L = C.POINTER(C.c_float), _l.load()
    if G is None:
        check(L.sfe_dsp_eig_plan(S, B, int(n_vec), M, pa, int(widely_linear), int(signal_dim), None, None, None, None, None))
        return None
    G = np.ascontiguousarray(np.asarray(G, dtype=np.float32).reshape(M, 2 * S, 2 * S))
    E = max(int(n_vec), 0)
    val, nul = np.empty((M, 2 * S), np.float32), np.empty((M, B), np.float32)
    vec, st = np.empty((M, 2 * E, 2 * S), np.float32), np.empty(M, np.int32)
    check(L.sfe_dsp_eig_plan(S, B, int(n_vec), M, pa, int(widely_linear), int(signal_dim), G.ctypes.data_as(fp), val.ctypes.data_as(fp),
                             nul.ctypes.data_as(fp), vec.ctypes.data_as(fp), st.ctypes.data_as(C.POINTER(C.c_int))))
    return val, nul, vec, st


class Eig(_Block):
    """Symmetric eigen-decomposition / MUSIC direction finder (sfe_dsp_eig_*): per row of Cov's output and band, the
    eigenvalues of the Gram matrix (descending), the MUSIC null spectrum of n_beams = B scan steering vectors against the
    noise subspace left by signal_dim real dimensions, and the n_vec = E leading eigenvectors as the real matrix Beam
    multiplies by.  steering is (M, B, S) complex, (B, S) for one band, or None (no beams: n_in and n_bands give the shape)."""
    _prefix = "eig"

    def __init__(self, steering, widely_linear=False, signal_dim=0, n_vec=0, n_in=None, n_bands=1, device=0):
        a, pa = _eig_steering(steering, n_in, n_bands)
        self.n_bands, self.n_beams, self.n_in = (int(v) for v in a.shape)
        self.widely_linear, self.n_vec = bool(widely_linear), int(n_vec)
        self._create(pa, self.n_in, self.n_beams, self.n_vec, self.n_bands, int(self.widely_linear), int(signal_dim), device)

    def set_steering(self, steering):
        """New scan vectors of the same shape, used from the next call on."""
        a, pa = _mvdr_steering(steering)
        if a.shape != (self.n_bands, self.n_beams, self.n_in):
            raise ValueError("set_steering: shape %s for a handle of %s" % (a.shape, (self.n_bands, self.n_beams, self.n_in)))
        check(self._fn("set_steering")(self._h, pa))

    def set_signal_dim(self, signal_dim):
        """A new signal-subspace dimension, used from the next call on."""
        check(self._fn("set_signal_dim")(self._h, int(signal_dim)))

    def process_stream(self, d_gram, n_rows, d_values, d_null=None, d_vectors=None, d_status=None, in_stride=None, values_stride=None,
                       null_stride=None, vectors_stride=None, status_stride=None, stream=None):
        """d_*: DeviceArray or raw device pointers.  Row j of band k is read at d_gram + k*in_stride + j*(2S)^2 floats
        (Cov's output; in_stride defaults to n_rows*(2S)^2); its eigenvalues go to d_values + j*values_stride + k*2S, its
        null spectrum to d_null + j*null_stride + k*B, its eigen-beams to d_vectors + j*vectors_stride + k*4ES, its status
        (int32) to d_status + j*status_stride + k; the output strides default to one row's block.  Returns the number of
        rows decomposed."""
        M, B, E, n2 = self.n_bands, self.n_beams, self.n_vec, 2 * self.n_in
        k = C.c_size_t(0)
        check(self._fn("process_stream")(
            self._h, self._ptr(d_gram), int(n_rows), int(n_rows) * n2 * n2 if in_stride is None else int(in_stride),
            self._ptr(d_values), M * n2 if values_stride is None else int(values_stride),
            self._ptr(d_null), M * B if null_stride is None else int(null_stride),
            self._ptr(d_vectors), M * 2 * E * n2 if vectors_stride is None else int(vectors_stride),
            self._ptr(d_status), M if status_stride is None else int(status_stride), C.byref(k), stream))
        return k.value

    def reset(self):
        raise AttributeError("Eig has no reset: it carries no state")

    def decompose(self, G):
        """Host convenience, computed on the GPU: G is (M, rows, 2S, 2S) float32 (Cov.gram's result; (M, 2S, 2S) and, for
        one band, (2S, 2S) are one row); returns (values (rows, M, 2S), null (rows, M, B), vectors (rows, M, 2E, 2S), all
        float32, status (rows, M) int32)."""
        M, B, E, n2 = self.n_bands, self.n_beams, self.n_vec, 2 * self.n_in
        G = np.ascontiguousarray(np.asarray(G, dtype=np.float32).reshape(M, -1, n2, n2))
        rows = G.shape[1]
        d_g, d_v = DeviceArray.from_numpy(G.ravel()), DeviceArray(max(1, rows * M * n2))
        d_n, d_e, d_s = DeviceArray(max(1, rows * M * B)), DeviceArray(max(1, rows * M * 2 * E * n2)), DeviceArray(max(1, rows * M))
        try:
            if rows:
                self.process_stream(d_g, rows, d_v, d_n, d_e, d_s)
            val = d_v.to_numpy(rows * M * n2).reshape(rows, M, n2)
            nul = d_n.to_numpy(rows * M * B).reshape(rows, M, B)
            vec = d_e.to_numpy(rows * M * 2 * E * n2).reshape(rows, M, 2 * E, n2)
            st = d_s.to_numpy(rows * M).view(np.int32).reshape(rows, M)
        finally:
            for d in (d_g, d_v, d_n, d_e, d_s):
                d.free()
        return np.ascontiguousarray(val), np.ascontiguousarray(nul), np.ascontiguousarray(vec), np.ascontiguousarray(st)


def _burst_preamble(preamble):
    """(preamble as a 1-D complex64 array, its float pointer)."""
    p = np.ascontiguousarray(np.asarray(preamble, dtype=np.complex64).ravel())
    return p, p.view(np.float32).ctypes.data_as(C.POINTER(C.c_float))


def burst_plan(preamble, sps, n_sym, lag, timing_mode=0, min_gate=0.0, x=None, idx=None, gate=None, n_bursts=None, start_base=0,
               start_step=0, given=None):
    """sfe_dsp_burst_plan (host only, no GPU): validates, and with x -- the complex samples of ONE stream -- demodulates
    n_bursts bursts by the law in float64: returns (symbols (n_bursts, n_sym) complex64, record (n_bursts, 8) float32,
    status (n_bursts,) int32), or None without x.  idx (uint32) and gate (float32) are host arrays of n_bursts entries or
    None; n_bursts defaults to len(idx), else 1.  given, (n_bursts, 8) float32: tau, f, theta, a are taken from it and the
    estimators are skipped.  Raises SfeError on arguments the block refuses."""
    p, pp = _burst_preamble(preamble)
    fp, L = C.POINTER(C.c_float), _l.load()
    head = (pp, p.size, int(sps), int(n_sym), int(lag), int(timing_mode), float(min_gate))
    if x is None:
        check(L.sfe_dsp_burst_plan(*head, None, 0, None, None, 0, 0, 0, None, None, None, None))
        return None
    x = np.ascontiguousarray(np.asarray(x, dtype=np.complex64).ravel())
    if idx is not None:
        idx = np.ascontiguousarray(idx, dtype=np.uint32).ravel()
    nb = int(n_bursts) if n_bursts is not None else (idx.size if idx is not None else 1)
    if gate is not None:
        gate = np.ascontiguousarray(gate, dtype=np.float32).ravel()
    if given is not None:
        given = np.ascontiguousarray(given, dtype=np.float32).reshape(nb, 8)
    for name, v in (("idx", idx), ("gate", gate)):
        if v is not None and v.size != nb:
            raise ValueError("burst_plan: %s has %d entries for %d bursts" % (name, v.size, nb))
    N = max(int(n_sym), 0)
    sym, rec, st = np.empty((nb, N), np.complex64), np.empty((nb, 8), np.float32), np.empty(nb, np.int32)
    check(L.sfe_dsp_burst_plan(*head, x.view(np.float32).ctypes.data_as(fp), x.size,
                               None if idx is None else idx.ctypes.data_as(C.POINTER(C.c_uint32)),
                               None if gate is None else gate.ctypes.data_as(fp), nb, int(start_base), int(start_step),
                               None if given is None else given.ctypes.data_as(fp), sym.view(np.float32).ctypes.data_as(fp),
                               rec.ctypes.data_as(fp), st.ctypes.data_as(C.POINTER(C.c_int))))
    return sym, rec, st


class Burst(_Block):
    """Feed-forward burst demodulator (sfe_dsp_burst_*): per burst, a window of one stream that starts where the
    correlator's peak says becomes n_sym symbol-rate samples -- timing (Oerder-Meyr), carrier frequency and phase
    (data-aided on the preamble) and amplitude corrected -- with a record (tau, f, theta, a, q, evm, 0, 0) and a status."""
    _prefix = "burst"

    def __init__(self, preamble, sps, n_sym, lag, timing_mode=0, min_gate=0.0, n_streams=1, device=0):
        p, pp = _burst_preamble(preamble)
        self.sps, self.n_sym, self.n_pre, self.lag = int(sps), int(n_sym), p.size, int(lag)
        self.timing_mode, self.n_streams = int(timing_mode), int(n_streams)
        self.in_u8 = False
        self._create(pp, p.size, self.sps, self.n_sym, self.lag, self.timing_mode, float(min_gate), self.n_streams, device)

    def set_input_format(self, fmt):
        """lib.FMT_F32 (cf32) or lib.FMT_U8 ((I,Q) byte pairs, converted on load)."""
        self._set_input_format(fmt)

    def set_gate(self, min_gate):
        """A new min_gate, used from the next call on."""
        check(self._fn("set_gate")(self._h, float(min_gate)))

    def process_stream(self, d_in, n_in, n_bursts, d_out, d_idx=None, d_gate=None, d_rec=None, d_status=None, start_base=0, start_step=0,
                       in_stride=None, idx_stride=None, gate_stride=None, out_stride=None, status_stride=None, stream=None):
        """d_*: DeviceArray or raw device pointers.  Burst b of stream s starts at start_base + b*start_step + the uint32
        at d_idx + s*idx_stride + b (0 without d_idx) of the n_in samples at d_in + s*in_stride, is gated by the float32 at
        d_gate + s*gate_stride + b, and writes n_sym cf32 symbols at d_out + (s*n_bursts + b)*out_stride, 8 float32 at
        d_rec + (s*n_bursts + b)*8 and an int32 at d_status + s*status_stride + b.  in_stride defaults to n_in, out_stride
        to n_sym and the other strides to n_bursts.  Returns n_bursts."""
        nb = int(n_bursts)
        k = C.c_size_t(0)
        check(self._fn("process_stream")(
            self._h, self._ptr(d_in), int(n_in), int(n_in) if in_stride is None else int(in_stride),
            self._ptr(d_idx), nb if idx_stride is None else int(idx_stride), self._ptr(d_gate), nb if gate_stride is None else int(gate_stride),
            nb, int(start_base), int(start_step), self._ptr(d_out), self.n_sym if out_stride is None else int(out_stride),
            self._ptr(d_rec), self._ptr(d_status), nb if status_stride is None else int(status_stride), C.byref(k), stream))
        return k.value

    def reset(self):
        raise AttributeError("Burst has no reset: it carries no state")

    def demodulate(self, x, idx=None, gate=None, n_bursts=None, start_base=0, start_step=0):
        """Host convenience, computed on the GPU: x is (n_streams, n) complex -- or, with FMT_U8, (n_streams, 2n) uint8
        (I,Q) pairs -- idx (uint32) and gate (float32) are (n_streams, n_bursts) or None; returns (symbols (n_streams,
        n_bursts, n_sym) complex64, record (n_streams, n_bursts, 8) float32, status (n_streams, n_bursts) int32)."""
        S, N = self.n_streams, self.n_sym
        if idx is not None:
            idx = np.ascontiguousarray(idx, dtype=np.uint32).reshape(S, -1)
        if gate is not None:
            gate = np.ascontiguousarray(gate, dtype=np.float32).reshape(S, -1)
        nb = int(n_bursts) if n_bursts is not None else (idx.shape[1] if idx is not None else (gate.shape[1] if gate is not None else 1))
        d_in, n = self._upload_input(x)
        held = [d_in]
        try:
            d_idx = d_gate = None
            if idx is not None:
                d_idx = DeviceArray.from_numpy(idx.view(np.float32).ravel())
                held.append(d_idx)
            if gate is not None:
                d_gate = DeviceArray.from_numpy(gate.ravel())
                held.append(d_gate)
            d_out, d_rec, d_st = DeviceArray(max(1, S * nb * N * 2)), DeviceArray(max(1, S * nb * 8)), DeviceArray(max(1, S * nb))
            held += [d_out, d_rec, d_st]
            if nb:
                self.process_stream(d_in, n, nb, d_out, d_idx, d_gate, d_rec, d_st, start_base, start_step)
            sym = d_out.to_numpy(S * nb * N * 2).view(np.complex64).reshape(S, nb, N)
            rec = d_rec.to_numpy(S * nb * 8).reshape(S, nb, 8)
            st = d_st.to_numpy(S * nb).view(np.int32).reshape(S, nb)
        finally:
            for d in held:
                d.free()
        return np.ascontiguousarray(sym), np.ascontiguousarray(rec), np.ascontiguousarray(st)


def _vit_code(gen, keep):
    """(n_gen, the generators' pointer, the pattern's pointer or None, its period P, what keeps them alive)."""
    g = np.ascontiguousarray(np.asarray(gen, dtype=np.uint32).ravel())
    if keep is None:
        return g.size, g.ctypes.data_as(C.POINTER(C.c_uint32)), None, 1, (g,)
    k = np.ascontiguousarray(np.asarray(keep, dtype=np.uint8))
    if k.ndim != 2 or k.shape[1] != g.size:
        raise ValueError("vit: keep must be (P, n_gen) = (P, %d), not %s" % (g.size, k.shape))
    return g.size, g.ctypes.data_as(C.POINTER(C.c_uint32)), k.ctypes.data_as(C.POINTER(C.c_uint8)), k.shape[0], (g, k)


def vit_encode(K, gen, bits, keep=None, terminated=True):
    """sfe_dsp_vit_encode (host only): the payload bits (0 / 1, one per item) through the convolutional encoder of constraint
    length K and generators gen, K - 1 zero bits appended when terminated, the positions keep[t mod P][j] == 0 left out:
    the kept coded bits as a uint8 array of 0 / 1."""
    n, gp, kp, P, _alive = _vit_code(gen, keep)
    b = np.ascontiguousarray(np.asarray(bits, dtype=np.uint8).ravel())
    L, u8p, k = _l.load(), C.POINTER(C.c_uint8), C.c_size_t(0)
    check(L.sfe_dsp_vit_encode(int(K), n, gp, kp, P, int(bool(terminated)), b.ctypes.data_as(u8p), b.size, None, C.byref(k)))
    coded = np.empty(k.value, np.uint8)
    check(L.sfe_dsp_vit_encode(int(K), n, gp, kp, P, int(bool(terminated)), b.ctypes.data_as(u8p), b.size, coded.ctypes.data_as(u8p), C.byref(k)))
    return coded


def vit_footprint(K, n_gen, n_info, terminated=True):
    """sfe_dsp_vit_footprint (host only): (LDS bytes of one burst's survivors and packed bits, whether its soft values are
    staged in LDS beside them, bursts per workgroup -- 0 where create refuses the shape)."""
    by, st, w = C.c_size_t(0), C.c_int(0), C.c_int(0)
    check(_l.load().sfe_dsp_vit_footprint(int(K), int(n_gen), int(bool(terminated)), int(n_info), C.byref(by), C.byref(st), C.byref(w)))
    return by.value, bool(st.value), w.value


def vit_plan(K, gen, n_info, keep=None, terminated=True, in_mode=_l.VIT_IN_SOFT, skip=0, x=None, status_in=None):
    """sfe_dsp_vit_plan (host only, no GPU): validates and, without x, returns n_soft.  With x -- (n_bursts, row) float32
    soft values with VIT_IN_SOFT, complex symbols with VIT_IN_BPSK / VIT_IN_QPSK -- it decodes every row by the law in
    float32: returns (bytes (n_bursts, ceil(n_info / 8)) uint8, record (n_bursts, 2) uint32 -- the metric's float32 word,
    the disagreement count -- and status (n_bursts,) int32).  These are the device's bits.  status_in: int32 per burst or
    None.  Raises SfeError on arguments the block refuses."""
    n, gp, kp, P, _alive = _vit_code(gen, keep)
    L, ns = _l.load(), C.c_size_t(0)
    head = (int(K), n, gp, kp, P, int(bool(terminated)), int(n_info), int(in_mode), int(skip))
    if x is None:
        check(L.sfe_dsp_vit_plan(*head, None, 0, None, 0, None, 0, None, None, C.byref(ns)))
        return ns.value
    x = np.asarray(x)
    x = np.ascontiguousarray(x.reshape(1, -1) if x.ndim == 1 else x, dtype=np.float32 if in_mode == _l.VIT_IN_SOFT else np.complex64)
    nb, nbytes = x.shape[0], (max(int(n_info), 0) + 7) // 8
    if status_in is not None:
        status_in = np.ascontiguousarray(status_in, dtype=np.int32).ravel()
        if status_in.size != nb:
            raise ValueError("vit_plan: status_in has %d entries for %d bursts" % (status_in.size, nb))
    by, rec, st = np.empty((nb, nbytes), np.uint8), np.empty((nb, 2), np.uint32), np.empty(nb, np.int32)
    check(L.sfe_dsp_vit_plan(*head, x.view(np.float32).ctypes.data_as(C.POINTER(C.c_float)), x.shape[1],
                             None if status_in is None else status_in.ctypes.data_as(C.POINTER(C.c_int)), nb,
                             by.ctypes.data_as(C.POINTER(C.c_uint8)), nbytes, rec.ctypes.data_as(C.POINTER(C.c_uint32)),
                             st.ctypes.data_as(C.POINTER(C.c_int)), C.byref(ns)))
    return by, rec, st


class Vit(_Block):
    """Soft-decision Viterbi decoder (sfe_dsp_vit_*): per burst, n_soft soft values -- float32, or the components of the
    symbols a Burst wrote -- become ceil(n_info / 8) payload bytes, a record (the end state's metric word, the count of
    positions that disagree with the decoded word) and a status.  The device's bits are vit_plan's."""
    _prefix = "vit"

    def __init__(self, K, gen, n_info, keep=None, terminated=True, in_mode=_l.VIT_IN_SOFT, skip=0, device=0):
        n, gp, kp, P, _alive = _vit_code(gen, keep)
        self.K, self.n_gen, self.n_info, self.in_mode, self.skip = int(K), n, int(n_info), int(in_mode), int(skip)
        self.n_bytes = (max(self.n_info, 0) + 7) // 8
        self._create(self.K, n, gp, kp, P, int(bool(terminated)), self.n_info, self.in_mode, self.skip, device)
        self.n_soft = vit_plan(K, gen, n_info, keep, terminated, in_mode, skip)
        # elements of the mode's type a burst's row holds at least
        self.row = self.n_soft if self.in_mode == _l.VIT_IN_SOFT else self.skip + (self.n_soft if self.in_mode == _l.VIT_IN_BPSK else (self.n_soft + 1) // 2)

    def process_stream(self, d_in, n_bursts, d_bits, d_rec=None, d_status=None, d_status_in=None, in_stride=None, out_stride=None, stream=None):
        """d_*: DeviceArray or raw device pointers.  Burst b reads its row at d_in + b*in_stride (elements of the input
        mode's type; default: the row's own length) and, with d_status_in, the int32 at d_status_in + b; it writes n_bytes
        bytes at d_bits + b*out_stride (bytes; default n_bytes), two words at d_rec + 2b and an int32 at d_status + b.
        Returns n_bursts."""
        k = C.c_size_t(0)
        check(self._fn("process_stream")(self._h, self._ptr(d_in), self.row if in_stride is None else int(in_stride), self._ptr(d_status_in),
                                         int(n_bursts), self._ptr(d_bits), self.n_bytes if out_stride is None else int(out_stride),
                                         self._ptr(d_rec), self._ptr(d_status), C.byref(k), stream))
        return k.value

    def reset(self):
        raise AttributeError("Vit has no reset: it carries no state")

    def decode(self, x, status_in=None):
        """Host convenience, computed on the GPU: x is (n_bursts, row) -- float32 soft values, or complex symbols with
        VIT_IN_BPSK / VIT_IN_QPSK; returns (bytes (n_bursts, n_bytes) uint8, record (n_bursts, 2) uint32, status (n_bursts,)
        int32), as vit_plan does."""
        x = np.asarray(x)
        x = np.ascontiguousarray(x.reshape(1, -1) if x.ndim == 1 else x, dtype=np.float32 if self.in_mode == _l.VIT_IN_SOFT else np.complex64)
        nb = x.shape[0]
        held = [DeviceArray.from_numpy(x.view(np.float32))]
        try:
            d_si = None
            if status_in is not None:
                d_si = DeviceArray.from_numpy(np.ascontiguousarray(status_in, dtype=np.int32).reshape(nb).view(np.float32))
                held.append(d_si)
            d_by, d_rec, d_st = DeviceArray(max(1, (nb * self.n_bytes + 3) // 4)), DeviceArray(max(1, 2 * nb)), DeviceArray(max(1, nb))
            held += [d_by, d_rec, d_st]
            if nb:
                self.process_stream(held[0], nb, d_by, d_rec, d_st, d_si, in_stride=x.shape[1])
            by = d_by.to_numpy().view(np.uint8)[:nb * self.n_bytes].reshape(nb, self.n_bytes)
            rec = d_rec.to_numpy(2 * nb).view(np.uint32).reshape(nb, 2)
            st = d_st.to_numpy(nb).view(np.int32)
        finally:
            for d in held:
                d.free()
        return np.ascontiguousarray(by), np.ascontiguousarray(rec), np.ascontiguousarray(st)


def _mod_shape(K, gen, n_info, keep, terminated, order, preamble, sps, taps, amp, out_fmt):
    """The shape arguments sfe_dsp_mod_plan and sfe_dsp_mod_create share, and what keeps their arrays alive.  gen None or
    empty: uncoded."""
    if gen is None or len(gen) == 0:
        n, gp, kp, P, alive = 0, None, None, 1, ()
    else:
        n, gp, kp, P, alive = _vit_code(gen, keep)
    p, pp = _burst_preamble(preamble if preamble is not None else [])
    t = np.ascontiguousarray(np.asarray(taps, dtype=np.float32).ravel())
    head = (int(K), n, gp, kp, P, int(bool(terminated)), int(n_info), int(order), pp if p.size else None, p.size, int(sps),
            t.ctypes.data_as(C.POINTER(C.c_float)), t.size, float(amp), int(out_fmt))
    return head, (alive, p, t)


def mod_footprint():
    """sfe_dsp_mod_footprint (host only): (samples of the stream one workgroup writes, the LDS bytes it uses)."""
    ts, by = C.c_int(0), C.c_size_t(0)
    check(_l.load().sfe_dsp_mod_footprint(C.byref(ts), C.byref(by)))
    return ts.value, by.value


def mod_plan(K, gen, n_info, taps, sps, keep=None, terminated=True, order=2, preamble=None, amp=1.0, out_fmt=_l.FMT_F32, data=None,
             n_out=0, start_base=0, start_step=0, n_bursts=None):
    """sfe_dsp_mod_plan (host only, no GPU): validates and, without data, returns (N symbols per burst, F samples per frame,
    n_soft) -- after checking the placement too where n_out or n_bursts is given.  With data -- (n_bursts, >= ceil(n_info / 8))
    uint8 payload bytes, MSB-first -- it writes the stream of n_out samples by the law: returns complex64 (n_out,), or the
    (n_out / 2) * 5 uint8 bytes of the transmit wire format with FMT_TX10.  These are the device's bits.  gen None: uncoded.
    Raises SfeError on arguments the block refuses."""
    head, _alive = _mod_shape(K, gen, n_info, keep, terminated, order, preamble, sps, taps, amp, out_fmt)
    L, N, F, ns = _l.load(), C.c_int(0), C.c_int(0), C.c_size_t(0)
    tail = (C.byref(N), C.byref(F), C.byref(ns))
    if data is None:
        check(L.sfe_dsp_mod_plan(*head, None, 0, int(n_bursts or 0), int(start_base), int(start_step), int(n_out), None, *tail))
        return N.value, F.value, ns.value
    d = np.asarray(data, dtype=np.uint8)
    d = np.ascontiguousarray(d.reshape(1, -1) if d.ndim == 1 else d)
    nb = d.shape[0] if n_bursts is None else int(n_bursts)
    n_out = max(int(n_out), 0)
    out = np.empty(n_out // 2 * 5, np.uint8) if out_fmt == _l.FMT_TX10 else np.empty(n_out, np.complex64)
    check(L.sfe_dsp_mod_plan(*head, d.ctypes.data_as(C.POINTER(C.c_uint8)), d.shape[1] if d.size else 0, nb, int(start_base), int(start_step),
                             n_out, out.ctypes.data if out.size else None, *tail))
    return out


class Mod(_Block):
    """Burst modulator (sfe_dsp_mod_*): per burst, ceil(n_info / 8) packed payload bytes on the device -- what a Vit wrote,
    say -- are encoded, mapped to BPSK or Gray QPSK behind a preamble, pulse-shaped and written as one frame of an output
    stream, cf32 or (out_fmt FMT_TX10) the transmit wire format; every other sample of the stream is written as zero.
    The device's bits are mod_plan's."""
    _prefix = "mod"

    def __init__(self, K, gen, n_info, taps, sps, keep=None, terminated=True, order=2, preamble=None, amp=1.0, out_fmt=_l.FMT_F32, device=0):
        head, _alive = _mod_shape(K, gen, n_info, keep, terminated, order, preamble, sps, taps, amp, out_fmt)
        self.n_info, self.sps, self.order, self.out_fmt = int(n_info), int(sps), int(order), int(out_fmt)
        self.n_bytes = (max(self.n_info, 0) + 7) // 8
        self._create(*head, device)
        self.n_sym, self.frame_len, self.n_soft = mod_plan(K, gen, n_info, taps, sps, keep, terminated, order, preamble, amp, out_fmt)

    def process_stream(self, d_bytes, n_bursts, d_out, n_out, start_base=0, start_step=0, in_stride=None, stream=None):
        """d_*: DeviceArray or raw device pointers.  Burst b reads n_bytes bytes at d_bytes + b*in_stride (bytes; default
        n_bytes) and its frame_len samples start at sample start_base + b*start_step of the n_out samples at d_out (cf32, or
        5-byte groups of two samples with FMT_TX10); the call writes all n_out samples.  Returns n_out."""
        k = C.c_size_t(0)
        check(self._fn("process_stream")(self._h, self._ptr(d_bytes), self.n_bytes if in_stride is None else int(in_stride), int(n_bursts),
                                         int(start_base), int(start_step), self._ptr(d_out), int(n_out), C.byref(k), stream))
        return k.value

    def reset(self):
        raise AttributeError("Mod has no reset: it carries no state")

    def modulate(self, data, n_out, start_base=0, start_step=0):
        """Host convenience, computed on the GPU: data is (n_bursts, n_bytes) uint8; returns what mod_plan returns."""
        d = np.asarray(data, dtype=np.uint8)
        d = np.ascontiguousarray(d.reshape(1, -1) if d.ndim == 1 else d)
        tx10 = self.out_fmt == _l.FMT_TX10
        nbytes = int(n_out) // 2 * 5 if tx10 else 8 * int(n_out)
        held = [DeviceArray.from_bytes(d), DeviceArray(max(1, (nbytes + 3) // 4))]
        try:
            self.process_stream(held[0], d.shape[0], held[1], n_out, start_base, start_step, in_stride=d.shape[1])
            raw = held[1].to_numpy().view(np.uint8)[:nbytes]
        finally:
            for x in held:
                x.free()
        return np.ascontiguousarray(raw) if tx10 else np.ascontiguousarray(raw).view(np.complex64)


def polar_plan(x, mode, gain, prev=None, in_u8=False):
    """sfe_dsp_polar_plan (host only, no GPU): the detector's law on one stream, bit for bit what the device computes.  x is
    (n,) complex64, or with in_u8 the 2n (I,Q) bytes; prev the carried sample (complex; None: a fresh stream).  Returns
    (y (n,) float32, the carried sample after x as complex64)."""
    if in_u8:
        a = np.ascontiguousarray(x, dtype=np.uint8).reshape(-1)
        n = a.size // 2
    else:
        a = np.ascontiguousarray(x, dtype=np.complex64).reshape(-1)
        n = a.size
    p = np.zeros(2, np.float32)
    if prev is not None:
        p[:] = (np.complex64(prev).real, np.complex64(prev).imag)
    y = np.empty(n, np.float32)
    check(_l.load().sfe_dsp_polar_plan(int(mode), float(gain), _l.FMT_U8 if in_u8 else _l.FMT_F32, a.ctypes.data if n else None, n,
                                       p.ctypes.data_as(_l.fp), y.ctypes.data_as(_l.fp)))
    return y, p.view(np.complex64)[0]


class Polar(_Block):
    """Streaming FM, phase and envelope detector (sfe_dsp_polar_*): one real float32 output per complex sample of each of
    n_streams streams; mode is lib.POLAR_FM (gain * angle of x[n] conj(x[n-1])), POLAR_PM (gain * angle of x[n]) or
    POLAR_AM (gain * |x[n]|).  Any call size; FM carries the last sample from call to call."""
    _prefix = "polar"

    def __init__(self, mode, gain=1.0, n_streams=1, device=0):
        self.mode, self.gain, self.n_streams = int(mode), float(gain), int(n_streams)
        self.in_u8 = False
        self._create(self.mode, self.gain, self.n_streams, device)

    def set_input_format(self, fmt):
        """lib.FMT_F32 (cf32) or lib.FMT_U8 ((I,Q) byte pairs, converted on load)."""
        self._set_input_format(fmt)

    def process_stream(self, d_in, n_in, d_out, in_stride=None, out_stride=None, stream=None):
        """d_in / d_out: DeviceArray or raw device pointers; n_in >= 1 samples per stream.  Stream s goes from
        d_in + s*in_stride samples of the input format to d_out + s*out_stride floats; both strides default to n_in.
        Returns n_out = n_in."""
        return self._process_stream(d_in, n_in, in_stride, d_out, int(n_in) if out_stride is None else out_stride, stream)

    def detect(self, x):
        """Host convenience, computed on the GPU, continuing the handle's state: x is (n_streams, n) complex64, or with
        FMT_U8 uint8 (I,Q) pairs with a last axis of 2n ((n,) / (2n,) for one stream).  Returns (n_streams, n) ((n,))
        float32."""
        one = self.n_streams == 1 and np.ndim(x) == 1
        d_in, n = self._upload_input(x)
        d_out = DeviceArray(max(1, self.n_streams * n))
        try:
            if n:
                self.process_stream(d_in, n, d_out)
            y = d_out.to_numpy(self.n_streams * n).reshape(self.n_streams, n)
        finally:
            d_in.free()
            d_out.free()
        return np.ascontiguousarray(y[0] if one else y)


# sfe_occ_info and sfe_occ_rec of include/sfe_dsp.h
OCC_INFO = np.dtype([("floor", "<f4"), ("thr", "<f4"), ("count", "<u4"), ("status", "<u4")])
OCC_REC = np.dtype([("lo", "<i4"), ("hi", "<i4"), ("peak", "<i4"), ("peak_val", "<f4"), ("sum", "<f4"), ("moment", "<f4"),
                    ("zero", "<u4", (2,))])


def _occ_params(n_bins, rank, factor, min_level, gap, min_width, max_emissions, shift):
    return (int(n_bins), int(rank), float(factor), float(min_level), int(gap), int(min_width), int(max_emissions), int(shift))


def occ_plan(rows, rank, factor, min_level=0.0, gap=0, min_width=1, max_emissions=16, shift=False, n_bins=None):
    """sfe_dsp_occ_plan (host only, no GPU): the occupancy detector's law on rows (..., n_bins) float32, byte for byte what
    the device computes.  Returns (info (rows,) OCC_INFO, rec (rows, max_emissions) OCC_REC, mask (rows, n_bins) uint8).
    Raises SfeError on parameters the block refuses; rows None (with n_bins) only validates them."""
    if rows is None:
        check(_l.load().sfe_dsp_occ_plan(*_occ_params(n_bins, rank, factor, min_level, gap, min_width, max_emissions, shift), None, 0, None,
                                         None, None))
        return None
    x = np.ascontiguousarray(rows, dtype=np.float32)
    x = x.reshape(1, -1) if x.ndim == 1 else x.reshape(-1, x.shape[-1])
    R, N = x.shape
    E = int(max_emissions)
    info, rec, mask = np.empty(R, OCC_INFO), np.empty((R, max(E, 0)), OCC_REC), np.empty((R, N), np.uint8)
    check(_l.load().sfe_dsp_occ_plan(*_occ_params(N, rank, factor, min_level, gap, min_width, E, shift), x.ctypes.data_as(_l.fp), R,
                                     info.ctypes.data, rec.ctypes.data, mask.ctypes.data))       # (the parameters are checked first)
    return info, rec, mask


class Occ(_Block):
    """Spectrum occupancy detector (sfe_dsp_occ_*): per row of n_bins float32 spectrum bins -- a Psd's rows where it left
    them -- the floor (the value of rank `rank`), the threshold max(factor * floor, min_level), and one record per emission
    (a run of bins above the threshold, gaps of at most `gap` bins closed, at least min_width wide): bounds and peak in
    signed bins, peak value, sum and first moment.  The device's bytes are occ_plan's.  Stateless: there is no reset."""
    _prefix = "occ"

    def __init__(self, n_bins, rank, factor, min_level=0.0, gap=0, min_width=1, max_emissions=16, shift=False, device=0):
        self.n_bins, self.max_emissions, self.shift = int(n_bins), int(max_emissions), bool(shift)
        self._create(*_occ_params(n_bins, rank, factor, min_level, gap, min_width, max_emissions, shift), device)

    def process_stream(self, d_in, n_rows, d_info, d_rec, d_mask=None, n_streams=1, in_stride=None, out_stride=None, stream=None):
        """d_*: DeviceArray or raw device pointers.  Row j of stream s is read at d_in + s*in_stride + j*n_bins floats
        (in_stride defaults to n_rows*n_bins) and goes to slot s*out_stride + j (out_stride defaults to n_rows) of d_info
        (16 bytes a slot), d_rec (32*max_emissions) and, if given, d_mask (n_bins).  Returns the rows done."""
        k = C.c_size_t(0)
        check(self._fn("process_stream")(self._h, self._ptr(d_in), int(n_streams), int(n_rows),
                                         int(n_rows) * self.n_bins if in_stride is None else int(in_stride), self._ptr(d_info),
                                         self._ptr(d_rec), self._ptr(d_mask), int(n_rows) if out_stride is None else int(out_stride),
                                         C.byref(k), stream))
        return k.value

    def reset(self):
        raise AttributeError("Occ has no reset: it carries no state")

    def detect(self, rows, mask=True):
        """Host convenience, computed on the GPU: rows is (..., n_bins) float32; returns what occ_plan returns (mask None
        without `mask`)."""
        x = np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, self.n_bins)
        R, N, E = x.shape[0], self.n_bins, self.max_emissions
        held = [DeviceArray.from_numpy(x), DeviceArray(max(1, 4 * R)), DeviceArray(max(1, 8 * E * R)), DeviceArray(max(1, (R * N + 3) // 4))]
        try:
            if R:
                self.process_stream(held[0], R, held[1], held[2], held[3] if mask else None)
            info = held[1].to_numpy(4 * R).view(OCC_INFO)
            rec = held[2].to_numpy(8 * E * R).view(OCC_REC).reshape(R, E)
            m = held[3].to_numpy().view(np.uint8)[:R * N].reshape(R, N) if mask else None
        finally:
            for d in held:
                d.free()
        return info, rec, (np.ascontiguousarray(m) if mask else None)


def _reed_shape(prim, fcr, step, n, n_par, depth, whiten):
    """The shape arguments sfe_dsp_reed_plan and sfe_dsp_reed_create share, and what keeps the whitening bytes alive."""
    w = None if whiten is None else np.ascontiguousarray(np.asarray(whiten, dtype=np.uint8).ravel())
    if w is not None and w.size != max(int(depth), 0) * max(int(n), 0):
        raise ValueError("reed: whiten has %d bytes for a frame of depth * n = %d" % (w.size, int(depth) * int(n)))
    return (int(prim), int(fcr), int(step), int(n), int(n_par), int(depth), None if w is None else w.ctypes.data), w


def reed_plan(prim, fcr, step, n, n_par, depth, whiten=None, data=None, encode=False, status_in=None):
    """sfe_dsp_reed_plan (host only, no GPU): validates and, without data, returns (payload_bytes, frame_bytes).  With data
    and encode -- (n_frames, >= payload_bytes) uint8 -- it returns the frames (n_frames, frame_bytes) uint8; with data and not
    encode -- (n_frames, >= frame_bytes) uint8 channel bytes -- it returns (bytes (n_frames, payload_bytes) uint8, record
    (n_frames, 2) uint32 -- the corrected byte count, the mask of uncorrectable codewords -- and status (n_frames,) int32).
    These are the device's bytes.  status_in: int32 per frame or None.  Raises SfeError on arguments the block refuses."""
    head, _alive = _reed_shape(prim, fcr, step, n, n_par, depth, whiten)
    L, P, Fb = _l.load(), C.c_int(0), C.c_int(0)
    if data is None:
        check(L.sfe_dsp_reed_plan(*head, int(bool(encode)), None, 0, None, 0, None, 0, None, None, C.byref(P), C.byref(Fb)))
        return P.value, Fb.value
    check(L.sfe_dsp_reed_plan(*head, int(bool(encode)), None, 0, None, 0, None, 0, None, None, C.byref(P), C.byref(Fb)))
    d = np.asarray(data, dtype=np.uint8)
    d = np.ascontiguousarray(d.reshape(1, -1) if d.ndim == 1 else d)
    nf = d.shape[0]
    if status_in is not None:
        status_in = np.ascontiguousarray(status_in, dtype=np.int32).ravel()
        if status_in.size != nf:
            raise ValueError("reed_plan: status_in has %d entries for %d frames" % (status_in.size, nf))
    out = np.empty((nf, Fb.value if encode else P.value), np.uint8)
    rec, st = np.empty((nf, 2), np.uint32), np.empty(nf, np.int32)
    check(L.sfe_dsp_reed_plan(*head, int(bool(encode)), d.ctypes.data if d.size else None, d.shape[1],
                              None if status_in is None else status_in.ctypes.data, nf, out.ctypes.data, out.shape[1], rec.ctypes.data,
                              st.ctypes.data, None, None))
    return out if encode else (out, rec, st)


class Reed(_Block):
    """Interleaved Reed-Solomon outer code over GF(2^8) (sfe_dsp_reed_*): encode_stream turns payload_bytes = depth * (n - n_par)
    bytes per frame into frame_bytes = depth * n channel bytes (in front of a Mod), process_stream turns channel bytes -- what
    a Vit wrote -- back into payloads, correcting up to t = n_par // 2 wrong bytes in each of a frame's `depth` codewords, with
    a record (bytes corrected, mask of uncorrectable codewords) and a status per frame.  The device's bytes are reed_plan's."""
    _prefix = "reed"

    def __init__(self, prim, fcr, step, n, n_par, depth, whiten=None, device=0):
        head, _alive = _reed_shape(prim, fcr, step, n, n_par, depth, whiten)
        self.n, self.n_par, self.depth, self.t = int(n), int(n_par), int(depth), int(n_par) // 2
        self._create(*head, device)
        self.payload_bytes, self.frame_bytes = self.depth * (self.n - self.n_par), self.depth * self.n

    def encode_stream(self, d_payload, n_frames, d_frame, in_stride=None, out_stride=None, stream=None):
        """d_*: DeviceArray or raw device pointers.  Frame b reads payload_bytes bytes at d_payload + b*in_stride (default
        payload_bytes) and writes frame_bytes bytes at d_frame + b*out_stride (default frame_bytes).  Returns n_frames."""
        k = C.c_size_t(0)
        check(self._fn("encode_stream")(self._h, self._ptr(d_payload), self.payload_bytes if in_stride is None else int(in_stride), int(n_frames),
                                        self._ptr(d_frame), self.frame_bytes if out_stride is None else int(out_stride), C.byref(k), stream))
        return k.value

    def process_stream(self, d_frame, n_frames, d_out, d_rec=None, d_status=None, d_status_in=None, in_stride=None, out_stride=None, stream=None):
        """d_*: DeviceArray or raw device pointers.  Frame b reads frame_bytes bytes at d_frame + b*in_stride (default
        frame_bytes) and, with d_status_in, the int32 at d_status_in + b; it writes payload_bytes bytes at d_out + b*out_stride
        (default payload_bytes), two words at d_rec + 2b and an int32 at d_status + b.  Returns n_frames."""
        k = C.c_size_t(0)
        check(self._fn("process_stream")(self._h, self._ptr(d_frame), self.frame_bytes if in_stride is None else int(in_stride),
                                         self._ptr(d_status_in), int(n_frames), self._ptr(d_out),
                                         self.payload_bytes if out_stride is None else int(out_stride), self._ptr(d_rec), self._ptr(d_status),
                                         C.byref(k), stream))
        return k.value

    def reset(self):
        raise AttributeError("Reed has no reset: it carries no state")

    def encode(self, data):
        """Host convenience, computed on the GPU: data is (n_frames, payload_bytes) uint8; returns (n_frames, frame_bytes)."""
        d = np.asarray(data, dtype=np.uint8)
        d = np.ascontiguousarray(d.reshape(1, -1) if d.ndim == 1 else d)
        nf = d.shape[0]
        held = [DeviceArray.from_bytes(d), DeviceArray(max(1, (nf * self.frame_bytes + 3) // 4))]
        try:
            if nf:
                self.encode_stream(held[0], nf, held[1], in_stride=d.shape[1])
            raw = held[1].to_numpy().view(np.uint8)[:nf * self.frame_bytes].reshape(nf, self.frame_bytes)
        finally:
            for x in held:
                x.free()
        return np.ascontiguousarray(raw)

    def decode(self, frames, status_in=None):
        """Host convenience, computed on the GPU: frames is (n_frames, frame_bytes) uint8; returns what reed_plan returns."""
        d = np.asarray(frames, dtype=np.uint8)
        d = np.ascontiguousarray(d.reshape(1, -1) if d.ndim == 1 else d)
        nf, P = d.shape[0], self.payload_bytes
        held = [DeviceArray.from_bytes(d), DeviceArray(max(1, (nf * P + 3) // 4)), DeviceArray(max(1, 2 * nf)), DeviceArray(max(1, nf))]
        try:
            d_si = None
            if status_in is not None:
                d_si = DeviceArray.from_numpy(np.ascontiguousarray(status_in, dtype=np.int32).reshape(nf).view(np.float32))
                held.append(d_si)
            if nf:
                self.process_stream(held[0], nf, held[1], held[2], held[3], d_si, in_stride=d.shape[1])
            by = held[1].to_numpy().view(np.uint8)[:nf * P].reshape(nf, P)
            rec = held[2].to_numpy(2 * nf).view(np.uint32).reshape(nf, 2)
            st = held[3].to_numpy(nf).view(np.int32)
        finally:
            for x in held:
                x.free()
        return np.ascontiguousarray(by), np.ascontiguousarray(rec), np.ascontiguousarray(st)


def _ldpc_shape(shift, Z):
    """(mb, nb, Z, the base matrix's pointer) as sfe_dsp_ldpc_* take them, and what keeps the matrix alive."""
    s = np.ascontiguousarray(np.asarray(shift, dtype=np.int16))
    if s.ndim != 2:
        raise ValueError("ldpc: the base matrix must be (mb, nb), not %s" % (s.shape,))
    return (s.shape[0], s.shape[1], int(Z), s.ctypes.data), s


def _ldpc_rows(x, in_mode):
    x = np.asarray(x)
    return np.ascontiguousarray(x.reshape(1, -1) if x.ndim == 1 else x, dtype=np.float32 if in_mode == _l.VIT_IN_SOFT else np.complex64)


def ldpc_footprint(shift, Z):
    """sfe_dsp_ldpc_footprint (host only): (LDS bytes of a decoding workgroup, the codewords it holds)."""
    head, _alive = _ldpc_shape(shift, Z)
    by, w = C.c_size_t(0), C.c_int(0)
    check(_l.load().sfe_dsp_ldpc_footprint(*head, C.byref(by), C.byref(w)))
    return by.value, w.value


def ldpc_plan(shift, Z, scale=8.0, a=12, beta=0, max_iter=32, in_mode=_l.VIT_IN_SOFT, skip=0, x=None, status_in=None, data=None):
    """sfe_dsp_ldpc_plan (host only, no GPU): validates and, without x and data, returns (n, k, encodable).  With x --
    (n_words, row) float32 soft values with VIT_IN_SOFT, complex symbols with VIT_IN_BPSK / VIT_IN_QPSK -- it decodes every
    row by the law: returns (bytes (n_words, ceil(k / 8)) uint8, record (n_words, 3) uint32 -- iterations, unsatisfied
    checks, decisions that left the input's sign -- and status (n_words,) int32).  With data -- (n_words, >= ceil(k / 8))
    uint8 payload bytes -- it encodes: returns the codewords (n_words, ceil(n / 8)) uint8.  These are the device's bytes.
    status_in: int32 per codeword or None.  Raises SfeError on arguments the block refuses."""
    head, _alive = _ldpc_shape(shift, Z)
    L, n, k, enc = _l.load(), C.c_int(0), C.c_int(0), C.c_int(0)
    head = (*head, float(scale), int(a), int(beta), int(max_iter), int(in_mode), int(skip))
    check(L.sfe_dsp_ldpc_plan(*head, 0, None, 0, None, 0, None, 0, None, None, C.byref(n), C.byref(k), C.byref(enc)))
    if x is None and data is None:
        return n.value, k.value, bool(enc.value)
    kb, nbytes = (k.value + 7) // 8, (n.value + 7) // 8
    if data is not None:
        d = np.asarray(data, dtype=np.uint8)
        d = np.ascontiguousarray(d.reshape(1, -1) if d.ndim == 1 else d)
        out = np.empty((d.shape[0], nbytes), np.uint8)
        check(L.sfe_dsp_ldpc_plan(*head, 1, d.ctypes.data if d.size else None, d.shape[1], None, d.shape[0], out.ctypes.data, nbytes, None, None,
                                  None, None, None))
        return out
    x = _ldpc_rows(x, in_mode)
    nw = x.shape[0]
    if status_in is not None:
        status_in = np.ascontiguousarray(status_in, dtype=np.int32).ravel()
        if status_in.size != nw:
            raise ValueError("ldpc_plan: status_in has %d entries for %d codewords" % (status_in.size, nw))
    by, rec, st = np.empty((nw, kb), np.uint8), np.empty((nw, 3), np.uint32), np.empty(nw, np.int32)
    check(L.sfe_dsp_ldpc_plan(*head, 0, x.ctypes.data if x.size else None, x.shape[1], None if status_in is None else status_in.ctypes.data, nw,
                              by.ctypes.data, kb, rec.ctypes.data, st.ctypes.data, None, None, None))
    return by, rec, st


class Ldpc(_Block):
    """Quasi-cyclic LDPC code (sfe_dsp_ldpc_*): encode_stream turns ceil(k / 8) payload bytes per codeword into ceil(n / 8)
    codeword bytes (in front of an uncoded Mod), process_stream turns n soft values per codeword -- float32, or the components
    of the symbols a Burst wrote -- back into payload bytes by layered min-sum decoding in integers, with a record
    (iterations, unsatisfied checks, decisions that left the input's sign) and a status per codeword.  The device's bytes are
    ldpc_plan's."""
    _prefix = "ldpc"

    def __init__(self, shift, Z, scale=8.0, a=12, beta=0, max_iter=32, in_mode=_l.VIT_IN_SOFT, skip=0, device=0):
        head, _alive = _ldpc_shape(shift, Z)
        self.in_mode, self.skip = int(in_mode), int(skip)
        self._create(*head, float(scale), int(a), int(beta), int(max_iter), self.in_mode, self.skip, device)
        self.n, self.k, self.encodable = ldpc_plan(shift, Z, scale, a, beta, max_iter, in_mode, skip)
        self.k_bytes, self.n_bytes = (self.k + 7) // 8, (self.n + 7) // 8
        # elements of the mode's type a codeword's row holds at least
        self.row = self.n if self.in_mode == _l.VIT_IN_SOFT else self.skip + (self.n if self.in_mode == _l.VIT_IN_BPSK else (self.n + 1) // 2)

    def encode_stream(self, d_payload, n_words, d_code, in_stride=None, out_stride=None, stream=None):
        """d_*: DeviceArray or raw device pointers.  Codeword b reads k_bytes bytes at d_payload + b*in_stride (default k_bytes)
        and writes n_bytes bytes at d_code + b*out_stride (default n_bytes).  Returns n_words."""
        k = C.c_size_t(0)
        check(self._fn("encode_stream")(self._h, self._ptr(d_payload), self.k_bytes if in_stride is None else int(in_stride), int(n_words),
                                        self._ptr(d_code), self.n_bytes if out_stride is None else int(out_stride), C.byref(k), stream))
        return k.value

    def process_stream(self, d_in, n_words, d_bits, d_rec=None, d_status=None, d_status_in=None, in_stride=None, out_stride=None, stream=None):
        """d_*: DeviceArray or raw device pointers.  Codeword b reads its row at d_in + b*in_stride (elements of the input
        mode's type; default: the row's own length) and, with d_status_in, the int32 at d_status_in + b; it writes k_bytes
        bytes at d_bits + b*out_stride (bytes; default k_bytes), three words at d_rec + 3b and an int32 at d_status + b.
        Returns n_words."""
        k = C.c_size_t(0)
        check(self._fn("process_stream")(self._h, self._ptr(d_in), self.row if in_stride is None else int(in_stride), self._ptr(d_status_in),
                                         int(n_words), self._ptr(d_bits), self.k_bytes if out_stride is None else int(out_stride),
                                         self._ptr(d_rec), self._ptr(d_status), C.byref(k), stream))
        return k.value

    def reset(self):
        raise AttributeError("Ldpc has no reset: it carries no state")

    def encode(self, data):
        """Host convenience, computed on the GPU: data is (n_words, k_bytes) uint8; returns (n_words, n_bytes)."""
        d = np.asarray(data, dtype=np.uint8)
        d = np.ascontiguousarray(d.reshape(1, -1) if d.ndim == 1 else d)
        nw = d.shape[0]
        held = [DeviceArray.from_bytes(d), DeviceArray(max(1, (nw * self.n_bytes + 3) // 4))]
        try:
            if nw:
                self.encode_stream(held[0], nw, held[1], in_stride=d.shape[1])
            raw = held[1].to_numpy().view(np.uint8)[:nw * self.n_bytes].reshape(nw, self.n_bytes)
        finally:
            for x in held:
                x.free()
        return np.ascontiguousarray(raw)

    def decode(self, x, status_in=None):
        """Host convenience, computed on the GPU: x is (n_words, row) -- float32 soft values, or complex symbols with
        VIT_IN_BPSK / VIT_IN_QPSK; returns what ldpc_plan returns."""
        x = _ldpc_rows(x, self.in_mode)
        nw, kb = x.shape[0], self.k_bytes
        held = [DeviceArray.from_numpy(x.view(np.float32)), DeviceArray(max(1, (nw * kb + 3) // 4)), DeviceArray(max(1, 3 * nw)), DeviceArray(max(1, nw))]
        try:
            d_si = None
            if status_in is not None:
                d_si = DeviceArray.from_numpy(np.ascontiguousarray(status_in, dtype=np.int32).reshape(nw).view(np.float32))
                held.append(d_si)
            if nw:
                self.process_stream(held[0], nw, held[1], held[2], held[3], d_si, in_stride=x.shape[1])
            by = held[1].to_numpy().view(np.uint8)[:nw * kb].reshape(nw, kb)
            rec = held[2].to_numpy(3 * nw).view(np.uint32).reshape(nw, 3)
            st = held[3].to_numpy(nw).view(np.int32)
        finally:
            for d in held:
                d.free()
        return np.ascontiguousarray(by), np.ascontiguousarray(rec), np.ascontiguousarray(st)


def _ofdm_shape(n_fft, cp, advance, n_train, n_data, kind, train, pilot, pilot_sign, cfo_mode, cfo_skip, out_mode, min_gate):
    """(the leading arguments of sfe_dsp_ofdm_plan / _create, the arrays they point into, Nd)."""
    fp = C.POINTER(C.c_float)
    kind = np.ascontiguousarray(kind, dtype=np.uint8).ravel()
    train = np.ascontiguousarray(np.asarray(train, dtype=np.complex64).ravel())
    pilot = None if pilot is None else np.ascontiguousarray(np.asarray(pilot, dtype=np.complex64).ravel())
    sign = None if pilot_sign is None else np.ascontiguousarray(pilot_sign, dtype=np.int8).ravel()
    for name, v, n in (("kind", kind, n_fft), ("train", train, n_fft), ("pilot", pilot, n_fft), ("pilot_sign", sign, n_data)):
        if v is not None and v.size != int(n) and int(n) > 0:
            raise ValueError("ofdm: %s has %d entries, not %d" % (name, v.size, int(n)))
    head = (int(n_fft), int(cp), int(advance), int(n_train), int(n_data), kind.ctypes.data, train.view(np.float32).ctypes.data_as(fp),
            None if pilot is None else pilot.view(np.float32).ctypes.data_as(fp), None if sign is None else sign.ctypes.data,
            int(cfo_mode), int(cfo_skip), int(out_mode), float(min_gate))
    return head, (kind, train, pilot, sign), int(np.count_nonzero(kind == 1))


def ofdm_plan(n_fft, cp, advance, n_train, n_data, kind, train, pilot=None, pilot_sign=None, cfo_mode=0, cfo_skip=0,
              out_mode=_l.OFDM_OUT_ZF, min_gate=0.0, x=None, idx=None, gate=None, n_bursts=None, start_base=0, start_step=0):
    """sfe_dsp_ofdm_plan (host only, no GPU): validates, and with x -- the complex samples of ONE stream -- receives
    n_bursts bursts by the law in float64: returns (symbols (n_bursts, n_data, Nd) complex64, chan (n_bursts, n_fft)
    complex64, record (n_bursts, 8) float32, status (n_bursts,) int32), or None without x.  idx (uint32) and gate
    (float32) are host arrays of n_bursts entries or None; n_bursts defaults to len(idx), else 1.  Raises SfeError on
    arguments the block refuses."""
    head, keep, Nd = _ofdm_shape(n_fft, cp, advance, n_train, n_data, kind, train, pilot, pilot_sign, cfo_mode, cfo_skip, out_mode, min_gate)
    fp, L = C.POINTER(C.c_float), _l.load()
    if x is None:
        check(L.sfe_dsp_ofdm_plan(*head, None, 0, None, None, 0, 0, 0, None, None, None, None))
        return None
    x = np.ascontiguousarray(np.asarray(x, dtype=np.complex64).ravel())
    if idx is not None:
        idx = np.ascontiguousarray(idx, dtype=np.uint32).ravel()
    nb = int(n_bursts) if n_bursts is not None else (idx.size if idx is not None else 1)
    if gate is not None:
        gate = np.ascontiguousarray(gate, dtype=np.float32).ravel()
    for name, v in (("idx", idx), ("gate", gate)):
        if v is not None and v.size != nb:
            raise ValueError("ofdm_plan: %s has %d entries for %d bursts" % (name, v.size, nb))
    Ns, N = max(int(n_data), 0), max(int(n_fft), 0)
    sym, ch = np.empty((nb, Ns, Nd), np.complex64), np.empty((nb, N), np.complex64)
    rec, st = np.empty((nb, 8), np.float32), np.empty(nb, np.int32)
    check(L.sfe_dsp_ofdm_plan(*head, x.view(np.float32).ctypes.data_as(fp), x.size,
                              None if idx is None else idx.ctypes.data_as(C.POINTER(C.c_uint32)),
                              None if gate is None else gate.ctypes.data_as(fp), nb, int(start_base), int(start_step),
                              sym.view(np.float32).ctypes.data_as(fp), ch.view(np.float32).ctypes.data_as(fp), rec.ctypes.data_as(fp),
                              st.ctypes.data_as(C.POINTER(C.c_int))))
    return sym, ch, rec, st


class Ofdm(_Block):
    """OFDM burst receiver (sfe_dsp_ofdm_*): per burst, a reach of n_train training and n_data data symbols that starts
    where the correlator's peak says becomes n_data rows of Nd equalised data-bin symbols -- frequency offset from the
    cyclic prefix, a per-bin channel estimate from the training symbols, the common phase from the pilots, zero-forcing or
    matched-filter output -- with the channel estimate, a record (eps, h2, min |H|^2 / h2, pilot error, arg phi_0,
    arg phi_last, 0, 0) and a status."""
    _prefix = "ofdm"

    def __init__(self, n_fft, cp, advance, n_train, n_data, kind, train, pilot=None, pilot_sign=None, cfo_mode=0, cfo_skip=0,
                 out_mode=_l.OFDM_OUT_ZF, min_gate=0.0, n_streams=1, device=0):
        head, _keep, self.n_data_bins = _ofdm_shape(n_fft, cp, advance, n_train, n_data, kind, train, pilot, pilot_sign, cfo_mode, cfo_skip,
                                                    out_mode, min_gate)
        self.n_fft, self.cp, self.advance, self.n_train, self.n_data = int(n_fft), int(cp), int(advance), int(n_train), int(n_data)
        self.n_sym = self.n_data * self.n_data_bins         # cf32 symbols a burst writes
        self.n_streams = int(n_streams)
        self.in_u8 = False
        self._create(*head, self.n_streams, device)

    def set_input_format(self, fmt):
        """lib.FMT_F32 (cf32) or lib.FMT_U8 ((I,Q) byte pairs, converted on load)."""
        self._set_input_format(fmt)

    def process_stream(self, d_in, n_in, n_bursts, d_out, d_idx=None, d_gate=None, d_chan=None, d_rec=None, d_status=None, start_base=0,
                       start_step=0, in_stride=None, idx_stride=None, gate_stride=None, out_stride=None, status_stride=None, stream=None):
        """d_*: DeviceArray or raw device pointers.  Burst b of stream s starts at start_base + b*start_step + the uint32
        at d_idx + s*idx_stride + b (0 without d_idx) of the n_in samples at d_in + s*in_stride, is gated by the float32 at
        d_gate + s*gate_stride + b, and writes n_data*Nd cf32 symbols at d_out + (s*n_bursts + b)*out_stride, n_fft cf32 at
        d_chan + (s*n_bursts + b)*n_fft, 8 float32 at d_rec + (s*n_bursts + b)*8 and an int32 at
        d_status + s*status_stride + b.  in_stride defaults to n_in, out_stride to n_data*Nd and the other strides to
        n_bursts.  Returns n_bursts."""
        nb = int(n_bursts)
        k = C.c_size_t(0)
        check(self._fn("process_stream")(
            self._h, self._ptr(d_in), int(n_in), int(n_in) if in_stride is None else int(in_stride),
            self._ptr(d_idx), nb if idx_stride is None else int(idx_stride), self._ptr(d_gate), nb if gate_stride is None else int(gate_stride),
            nb, int(start_base), int(start_step), self._ptr(d_out), self.n_sym if out_stride is None else int(out_stride),
            self._ptr(d_chan), self._ptr(d_rec), self._ptr(d_status), nb if status_stride is None else int(status_stride), C.byref(k), stream))
        return k.value

    def reset(self):
        raise AttributeError("Ofdm has no reset: it carries no state")

    def receive(self, x, idx=None, gate=None, n_bursts=None, start_base=0, start_step=0):
        """Host convenience, computed on the GPU: x is (n_streams, n) complex -- or, with FMT_U8, (n_streams, 2n) uint8
        (I,Q) pairs -- idx (uint32) and gate (float32) are (n_streams, n_bursts) or None; returns (symbols (n_streams,
        n_bursts, n_data, Nd) complex64, chan (n_streams, n_bursts, n_fft) complex64, record (n_streams, n_bursts, 8)
        float32, status (n_streams, n_bursts) int32)."""
        S, M, N = self.n_streams, self.n_sym, self.n_fft
        if idx is not None:
            idx = np.ascontiguousarray(idx, dtype=np.uint32).reshape(S, -1)
        if gate is not None:
            gate = np.ascontiguousarray(gate, dtype=np.float32).reshape(S, -1)
        nb = int(n_bursts) if n_bursts is not None else (idx.shape[1] if idx is not None else (gate.shape[1] if gate is not None else 1))
        d_in, n = self._upload_input(x)
        held = [d_in]
        try:
            d_idx = d_gate = None
            if idx is not None:
                d_idx = DeviceArray.from_numpy(idx.view(np.float32).ravel())
                held.append(d_idx)
            if gate is not None:
                d_gate = DeviceArray.from_numpy(gate.ravel())
                held.append(d_gate)
            d_out, d_ch = DeviceArray(max(1, S * nb * M * 2)), DeviceArray(max(1, S * nb * N * 2))
            d_rec, d_st = DeviceArray(max(1, S * nb * 8)), DeviceArray(max(1, S * nb))
            held += [d_out, d_ch, d_rec, d_st]
            if nb:
                self.process_stream(d_in, n, nb, d_out, d_idx, d_gate, d_ch, d_rec, d_st, start_base, start_step)
            sym = d_out.to_numpy(S * nb * M * 2).view(np.complex64).reshape(S, nb, self.n_data, self.n_data_bins)
            ch = d_ch.to_numpy(S * nb * N * 2).view(np.complex64).reshape(S, nb, N)
            rec = d_rec.to_numpy(S * nb * 8).reshape(S, nb, 8)
            st = d_st.to_numpy(S * nb).view(np.int32).reshape(S, nb)
        finally:
            for d in held:
                d.free()
        return np.ascontiguousarray(sym), np.ascontiguousarray(ch), np.ascontiguousarray(rec), np.ascontiguousarray(st)


def _ofdmmod_shape(n_fft, cp, n_train, n_data, kind, train, pilot, pilot_sign, amp, order, in_mode, out_fmt):
    """(the leading arguments of sfe_dsp_ofdmmod_plan / _create, the arrays they point into)."""
    head, keep, _nd = _ofdm_shape(n_fft, cp, 0, n_train, n_data, kind, train, pilot, pilot_sign, 0, 0, 0, 0.0)
    return (head[0], head[1], *head[3:9], float(amp), int(order), int(in_mode), int(out_fmt)), keep


def _ofdmmod_rows(data, symbols):
    """The input of a call as (n_bursts, stride) rows: complex64 in SYMBOLS mode, uint8 in BITS mode."""
    d = np.asarray(data, dtype=np.complex64 if symbols else np.uint8)
    return np.ascontiguousarray(d.reshape(1, -1) if d.ndim == 1 else d)


def ofdmmod_footprint(n_fft):
    """sfe_dsp_ofdmmod_footprint (host only): (lanes of a symbol's workgroup, samples in no frame one workgroup writes, the
    LDS bytes of a symbol's workgroup)."""
    nt, zt, by = C.c_int(0), C.c_int(0), C.c_size_t(0)
    check(_l.load().sfe_dsp_ofdmmod_footprint(int(n_fft), C.byref(nt), C.byref(zt), C.byref(by)))
    return nt.value, zt.value, by.value


def ofdmmod_plan(n_fft, cp, n_train, n_data, kind, train, pilot=None, pilot_sign=None, amp=1.0, order=4, in_mode=_l.OFDMMOD_IN_BITS,
                 out_fmt=_l.FMT_F32, data=None, n_out=0, start_base=0, start_step=0, n_bursts=None):
    """sfe_dsp_ofdmmod_plan (host only, no GPU): validates and, without data, returns (Nd data bins, F samples per frame, the
    bytes -- BITS mode -- or cf32 symbols -- SYMBOLS mode -- a burst reads), after checking the placement too where n_out or
    n_bursts is given.  With data -- (n_bursts, stride) uint8 coded bytes, MSB-first, or complex64 symbols -- it writes the
    stream of n_out samples by the law: returns complex64 (n_out,), or the (n_out / 2) * 5 uint8 bytes of the transmit wire
    format with FMT_TX10.  These are the device's bits.  Raises SfeError on arguments the block refuses."""
    head, _alive = _ofdmmod_shape(n_fft, cp, n_train, n_data, kind, train, pilot, pilot_sign, amp, order, in_mode, out_fmt)
    L, Nd, F, ni = _l.load(), C.c_int(0), C.c_int(0), C.c_size_t(0)
    tail = (C.byref(Nd), C.byref(F), C.byref(ni))
    if data is None:
        check(L.sfe_dsp_ofdmmod_plan(*head, None, 0, int(n_bursts or 0), int(start_base), int(start_step), int(n_out), None, *tail))
        return Nd.value, F.value, ni.value
    d = _ofdmmod_rows(data, in_mode == _l.OFDMMOD_IN_SYMBOLS)
    nb = d.shape[0] if n_bursts is None else int(n_bursts)
    n_out = max(int(n_out), 0)
    out = np.empty(n_out // 2 * 5, np.uint8) if out_fmt == _l.FMT_TX10 else np.empty(n_out, np.complex64)
    check(L.sfe_dsp_ofdmmod_plan(*head, d.ctypes.data if d.size else None, d.shape[1] if d.size else 0, nb, int(start_base), int(start_step), n_out,
                                 out.ctypes.data if out.size else None, *tail))
    return out


class OfdmMod(_Block):
    """OFDM burst modulator (sfe_dsp_ofdmmod_*), the transmit side of Ofdm: per burst, a row of coded bytes on the device --
    what Ldpc.encode_stream wrote, say -- or of cf32 symbols -- a row of Ofdm's output -- is mapped to the data bins of
    n_data symbols behind n_train training symbols, transformed, given its cyclic prefixes and written as one frame of an
    output stream, cf32 or (out_fmt FMT_TX10) the transmit wire format; every other sample of the stream is written as
    zero.  The device's bits are ofdmmod_plan's."""
    _prefix = "ofdmmod"

    def __init__(self, n_fft, cp, n_train, n_data, kind, train, pilot=None, pilot_sign=None, amp=1.0, order=4, in_mode=_l.OFDMMOD_IN_BITS,
                 out_fmt=_l.FMT_F32, device=0):
        head, _alive = _ofdmmod_shape(n_fft, cp, n_train, n_data, kind, train, pilot, pilot_sign, amp, order, in_mode, out_fmt)
        self.n_fft, self.cp, self.n_train, self.n_data = int(n_fft), int(cp), int(n_train), int(n_data)
        self.order, self.in_mode, self.out_fmt = int(order), int(in_mode), int(out_fmt)
        self._create(*head, device)
        self.n_data_bins, self.frame_len, self.n_in = ofdmmod_plan(n_fft, cp, n_train, n_data, kind, train, pilot, pilot_sign, amp, order,
                                                                   in_mode, out_fmt)
        self.n_sym = self.n_data * self.n_data_bins         # data symbols of a burst
        self.n_bytes = (self.n_sym * (2 if self.order == 4 else 1) + 7) // 8       # coded bytes of a burst in BITS mode

    def process_stream(self, d_in, n_bursts, d_out, n_out, start_base=0, start_step=0, in_stride=None, stream=None):
        """d_*: DeviceArray or raw device pointers.  Burst b reads n_bytes bytes (BITS mode) or n_sym cf32 (SYMBOLS mode) at
        d_in + b*in_stride (bytes or cf32; default: what a burst reads) and its frame_len samples start at sample
        start_base + b*start_step of the n_out samples at d_out (cf32, or 5-byte groups of two samples with FMT_TX10); the
        call writes all n_out samples.  Returns n_out."""
        k = C.c_size_t(0)
        check(self._fn("process_stream")(self._h, self._ptr(d_in), self.n_in if in_stride is None else int(in_stride), int(n_bursts),
                                         int(start_base), int(start_step), self._ptr(d_out), int(n_out), C.byref(k), stream))
        return k.value

    def reset(self):
        raise AttributeError("OfdmMod has no reset: it carries no state")

    def modulate(self, data, n_out, start_base=0, start_step=0):
        """Host convenience, computed on the GPU: data is (n_bursts, stride) uint8 coded bytes or complex64 symbols; returns
        what ofdmmod_plan returns."""
        symbols = self.in_mode == _l.OFDMMOD_IN_SYMBOLS
        d = _ofdmmod_rows(data, symbols)
        tx10 = self.out_fmt == _l.FMT_TX10
        nbytes = int(n_out) // 2 * 5 if tx10 else 8 * int(n_out)
        held = [DeviceArray.from_numpy(d.view(np.float32).ravel()) if symbols else DeviceArray.from_bytes(d), DeviceArray(max(1, (nbytes + 3) // 4))]
        try:
            self.process_stream(held[0], d.shape[0], held[1], n_out, start_base, start_step, in_stride=d.shape[1])
            raw = held[1].to_numpy().view(np.uint8)[:nbytes]
        finally:
            for x in held:
                x.free()
        return np.ascontiguousarray(raw) if tx10 else np.ascontiguousarray(raw).view(np.complex64)


def _qam_shape(order, amp, scale, n_sym, perm, csi_index, csi_len):
    """(the leading arguments of sfe_dsp_qam_plan / _create, the arrays they point into)."""
    perm = None if perm is None else np.ascontiguousarray(perm, dtype=np.uint32).ravel()
    idx = None if csi_index is None else np.ascontiguousarray(csi_index, dtype=np.uint32).ravel()
    head = (int(order), float(amp), float(scale), int(n_sym), None if perm is None else perm.ctypes.data,
            0 if idx is None else idx.size, int(csi_len), None if idx is None else idx.ctypes.data)
    return head, (perm, idx)


def qam_plan(order, n_sym, amp=1.0, scale=1.0, perm=None, csi_index=None, csi_len=0, data=None, sym=None, csi=None):
    """sfe_dsp_qam_plan (host only, no GPU): validates and, without data and sym, returns (bps, the bytes of a row of coded
    bits).  With data -- (n_rows, >= row bytes) uint8 coded bytes, MSB-first -- it maps: returns (n_rows, n_sym) complex64.
    With sym -- (n_rows, >= n_sym) complex64 -- and, on a shape with csi_index, csi -- (n_rows, >= csi_len) complex64 -- it
    demaps: returns (n_rows, n_sym * bps) float32 max-log soft values, positive for bit 0.  These are the device's bits.
    perm: uint32 [n_sym * bps], position t holds coded bit perm[t]; csi_index: uint32 [csi_period], each below csi_len.
    Raises SfeError on arguments the block refuses."""
    head, _alive = _qam_shape(order, amp, scale, n_sym, perm, csi_index, csi_len)
    L, bps, nb = _l.load(), C.c_int(0), C.c_size_t(0)
    tail = (C.byref(bps), C.byref(nb))
    check(L.sfe_dsp_qam_plan(*head, _l.QAM_MAP, None, 0, None, 0, 0, None, 0, *tail))
    if data is None and sym is None:
        return bps.value, nb.value
    n_sym = int(n_sym)
    if data is not None:
        d = np.asarray(data, dtype=np.uint8)
        d = np.ascontiguousarray(d.reshape(1, -1) if d.ndim == 1 else d)
        out = np.empty((d.shape[0], n_sym), np.complex64)
        check(L.sfe_dsp_qam_plan(*head, _l.QAM_MAP, d.ctypes.data if d.size else None, d.shape[1], None, 0, d.shape[0],
                                 out.ctypes.data if out.size else None, n_sym, *tail))
        return out
    z = np.asarray(sym, dtype=np.complex64)
    z = np.ascontiguousarray(z.reshape(1, -1) if z.ndim == 1 else z)
    h = None
    if csi is not None:
        h = np.asarray(csi, dtype=np.complex64)
        h = np.ascontiguousarray(h.reshape(1, -1) if h.ndim == 1 else h)
        if h.shape[0] != z.shape[0]:
            raise ValueError("qam_plan: csi has %d rows for %d rows of symbols" % (h.shape[0], z.shape[0]))
    out = np.empty((z.shape[0], n_sym * bps.value), np.float32)
    check(L.sfe_dsp_qam_plan(*head, _l.QAM_DEMAP, z.ctypes.data if z.size else None, z.shape[1], None if h is None else h.ctypes.data,
                             0 if h is None else h.shape[1], z.shape[0], out.ctypes.data if out.size else None, n_sym * bps.value, *tail))
    return out


class Qam(_Block):
    """QAM mapper and soft demapper (sfe_dsp_qam_*): map_stream turns rows of coded bytes on the device -- what
    Ldpc.encode_stream wrote -- into rows of cf32 constellation points of order 2, 4, 16, 64 or 256 for OfdmMod's SYMBOLS
    mode; demap_stream turns rows of cf32 equalised symbols -- a row of Ofdm's zero-forcing output -- into rows of float32
    max-log soft values for Ldpc / Vit in VIT_IN_SOFT mode, each symbol weighted by scale * |H|^2 read from Ofdm's d_chan
    through csi_index where one is given.  perm is an optional bit interleaver per row.  The device's bits are qam_plan's."""
    _prefix = "qam"

    def __init__(self, order, n_sym, amp=1.0, scale=1.0, perm=None, csi_index=None, csi_len=0, device=0):
        head, _alive = _qam_shape(order, amp, scale, n_sym, perm, csi_index, csi_len)
        self.order, self.n_sym = int(order), int(n_sym)
        self.csi_period, self.csi_len = head[5], int(csi_len) if head[5] else 0
        self._create(*head, device)
        self.bps, self.n_bytes = qam_plan(order, n_sym, amp, scale)
        self.n_bits = self.n_sym * self.bps         # floats a row of soft values holds

    def map_stream(self, d_bytes, n_rows, d_sym, in_stride=None, out_stride=None, stream=None):
        """d_*: DeviceArray or raw device pointers.  Row r reads n_bytes bytes at d_bytes + r*in_stride (bytes; default
        n_bytes) and writes n_sym cf32 at d_sym + r*out_stride (cf32; default n_sym).  Returns n_rows."""
        k = C.c_size_t(0)
        check(self._fn("map_stream")(self._h, self._ptr(d_bytes), self.n_bytes if in_stride is None else int(in_stride), int(n_rows),
                                     self._ptr(d_sym), self.n_sym if out_stride is None else int(out_stride), C.byref(k), stream))
        return k.value

    def demap_stream(self, d_sym, n_rows, d_soft, d_csi=None, in_stride=None, csi_stride=None, out_stride=None, stream=None):
        """d_*: DeviceArray or raw device pointers.  Row r reads n_sym cf32 at d_sym + r*in_stride (cf32; default n_sym) and,
        on a handle with csi_index, csi_len cf32 at d_csi + r*csi_stride (cf32; default csi_len); it writes n_bits floats at
        d_soft + r*out_stride (floats; default n_bits).  Returns n_rows."""
        k = C.c_size_t(0)
        check(self._fn("demap_stream")(self._h, self._ptr(d_sym), self.n_sym if in_stride is None else int(in_stride), self._ptr(d_csi),
                                       self.csi_len if csi_stride is None else int(csi_stride), int(n_rows), self._ptr(d_soft),
                                       self.n_bits if out_stride is None else int(out_stride), C.byref(k), stream))
        return k.value

    def reset(self):
        raise AttributeError("Qam has no reset: it carries no state")

    def map(self, data):
        """Host convenience, computed on the GPU: data is (n_rows, >= n_bytes) uint8; returns what qam_plan returns."""
        d = np.asarray(data, dtype=np.uint8)
        d = np.ascontiguousarray(d.reshape(1, -1) if d.ndim == 1 else d)
        nr = d.shape[0]
        held = [DeviceArray.from_bytes(d), DeviceArray(max(1, 2 * nr * self.n_sym))]
        try:
            if nr:
                self.map_stream(held[0], nr, held[1], in_stride=d.shape[1])
            out = held[1].to_numpy(2 * nr * self.n_sym).view(np.complex64).reshape(nr, self.n_sym)
        finally:
            for x in held:
                x.free()
        return np.ascontiguousarray(out)

    def demap(self, sym, csi=None):
        """Host convenience, computed on the GPU: sym is (n_rows, >= n_sym) complex64, csi (n_rows, >= csi_len) complex64 on a
        handle with csi_index; returns what qam_plan returns."""
        z = np.asarray(sym, dtype=np.complex64)
        z = np.ascontiguousarray(z.reshape(1, -1) if z.ndim == 1 else z)
        nr = z.shape[0]
        held = [DeviceArray.from_numpy(z.view(np.float32)), DeviceArray(max(1, nr * self.n_bits))]
        try:
            d_csi, cs = None, None
            if csi is not None:
                h = np.asarray(csi, dtype=np.complex64)
                h = np.ascontiguousarray(h.reshape(1, -1) if h.ndim == 1 else h)
                d_csi, cs = DeviceArray.from_numpy(h.view(np.float32)), h.shape[1]
                held.append(d_csi)
            if nr:
                self.demap_stream(held[0], nr, held[1], d_csi, in_stride=z.shape[1], csi_stride=cs)
            out = held[1].to_numpy(nr * self.n_bits).reshape(nr, self.n_bits)
        finally:
            for x in held:
                x.free()
        return np.ascontiguousarray(out)


def _fsk_shape(sps, pulse, h, pre, n_bits, mf, delay, rng, amp, scale, min_gate, out_fmt):
    """(the leading arguments of sfe_dsp_fsk_plan / _create, the arrays they point into)."""
    g = np.ascontiguousarray(np.asarray(pulse, dtype=np.float32).ravel())
    p = np.ascontiguousarray(np.asarray(pre, dtype=np.uint8).ravel())
    m = np.ascontiguousarray(np.asarray(mf, dtype=np.float32).ravel())
    head = (int(sps), g.ctypes.data if g.size else None, g.size, float(h), float(amp), p.ctypes.data if p.size else None, p.size, int(n_bits),
            m.ctypes.data if m.size else None, m.size, int(delay), int(rng), float(scale), float(min_gate), int(out_fmt))
    return head, (g, p, m)


def fsk_plan(sps, pulse, h, pre, n_bits, mf, delay, rng, amp=1.0, scale=1.0, min_gate=0.0, out_fmt=_l.FMT_F32, data=None, n_out=0,
             start_base=0, start_step=0, n_bursts=None, x=None, idx=None, gate=None, want_bits=True):
    """sfe_dsp_fsk_plan (host only, no GPU): validates and, without data and x, returns (N symbols per burst, F samples per
    frame, e (n_pre,) float32, den) -- after checking the placement too where n_out or n_bursts is given.  With data --
    (n_bursts, >= ceil(n_bits / 8)) uint8 payload bytes, MSB-first -- it modulates: returns the stream of n_out samples,
    complex64 (n_out,), or the (n_out / 2) * 5 uint8 bytes of the transmit wire format with FMT_TX10.  With x -- the complex
    samples of ONE stream -- it demodulates n_bursts bursts: returns (soft (n_bursts, n_bits) float32, bits (n_bursts,
    ceil(n_bits / 8)) uint8 or None, record (n_bursts, 8) float32, status (n_bursts,) int32); idx (uint32) and gate (float32)
    are host arrays of n_bursts entries or None; n_bursts defaults to len(idx), else 1.  These are the device's bits.
    Raises SfeError on arguments the block refuses."""
    head, _alive = _fsk_shape(sps, pulse, h, pre, n_bits, mf, delay, rng, amp, scale, min_gate, out_fmt)
    L, N, F, den = _l.load(), C.c_int(0), C.c_int(0), C.c_float(0.0)
    e = np.zeros(max(head[6], 1), np.float32)
    tail = (C.byref(N), C.byref(F), e.ctypes.data, C.byref(den))
    if data is None and x is None:
        check(L.sfe_dsp_fsk_plan(*head, _l.FSK_MOD, None, 0, None, None, int(n_bursts or 0), int(start_base), int(start_step), None, int(n_out),
                                 None, None, None, *tail))
        return N.value, F.value, e[:head[6]].copy(), den.value
    if data is not None:
        d = np.asarray(data, dtype=np.uint8)
        d = np.ascontiguousarray(d.reshape(1, -1) if d.ndim == 1 else d)
        nb = d.shape[0] if n_bursts is None else int(n_bursts)
        n_out = max(int(n_out), 0)
        out = np.empty(n_out // 2 * 5, np.uint8) if out_fmt == _l.FMT_TX10 else np.empty(n_out, np.complex64)
        check(L.sfe_dsp_fsk_plan(*head, _l.FSK_MOD, d.ctypes.data if d.size else None, d.shape[1] if d.size else 0, None, None, nb, int(start_base),
                                 int(start_step), out.ctypes.data if out.size else None, n_out, None, None, None, *tail))
        return out
    x = np.ascontiguousarray(np.asarray(x, dtype=np.complex64).ravel())
    if idx is not None:
        idx = np.ascontiguousarray(idx, dtype=np.uint32).ravel()
    if gate is not None:
        gate = np.ascontiguousarray(gate, dtype=np.float32).ravel()
    nb = int(n_bursts) if n_bursts is not None else (idx.size if idx is not None else 1)
    for name, v in (("idx", idx), ("gate", gate)):
        if v is not None and v.size != nb:
            raise ValueError("fsk_plan: %s has %d entries for %d bursts" % (name, v.size, nb))
    nbits = max(int(n_bits), 0)
    soft, rec, st = np.empty((nb, nbits), np.float32), np.empty((nb, 8), np.float32), np.empty(nb, np.int32)
    by = np.empty((nb, (nbits + 7) // 8), np.uint8) if want_bits else None
    check(L.sfe_dsp_fsk_plan(*head, _l.FSK_DEMOD, x.ctypes.data if x.size else None, x.size, None if idx is None else idx.ctypes.data,
                             None if gate is None else gate.ctypes.data, nb, int(start_base), int(start_step), soft.ctypes.data if soft.size else None,
                             0, None if by is None else by.ctypes.data, rec.ctypes.data, st.ctypes.data, *tail))
    return soft, by, rec, st


class Fsk(_Block):
    """2-(G)FSK burst modem (sfe_dsp_fsk_*): mod turns per burst ceil(n_bits / 8) coded bytes on the device -- what
    Ldpc.encode_stream or Reed.encode_stream wrote -- into one continuous-phase frame behind a preamble, placed in an output
    stream as Mod places its frames; demod turns per burst a window of a stream that starts where Corr's peak says into
    float32 soft values for Vit / Ldpc in VIT_IN_SOFT mode and, where asked, packed hard bits for Reed, with a record (tau, f,
    dev, q, 0, 0, 0, 0) and a status.  The device's bits are fsk_plan's."""
    _prefix = "fsk"

    def __init__(self, sps, pulse, h, pre, n_bits, mf, delay, rng, amp=1.0, scale=1.0, min_gate=0.0, out_fmt=_l.FMT_F32, n_streams=1, device=0):
        head, _alive = _fsk_shape(sps, pulse, h, pre, n_bits, mf, delay, rng, amp, scale, min_gate, out_fmt)
        self.sps, self.n_bits, self.n_pre, self.out_fmt, self.n_streams = int(sps), int(n_bits), head[6], int(out_fmt), int(n_streams)
        self.n_bytes = (max(self.n_bits, 0) + 7) // 8
        self.in_u8 = False
        self._create(*head, self.n_streams, device)
        self.n_sym, self.frame_len, self.e, self.den = fsk_plan(sps, pulse, h, pre, n_bits, mf, delay, rng, amp, scale, min_gate, out_fmt)

    def set_input_format(self, fmt):
        """The demodulator's input: lib.FMT_F32 (cf32) or lib.FMT_U8 ((I,Q) byte pairs, converted on load)."""
        self._set_input_format(fmt)

    def mod(self, d_bytes, n_bursts, d_out, n_out, start_base=0, start_step=0, in_stride=None, stream=None):
        """d_*: DeviceArray or raw device pointers.  Burst b reads n_bytes bytes at d_bytes + b*in_stride (bytes; default
        n_bytes) and its frame_len samples start at sample start_base + b*start_step of the n_out samples at d_out (cf32, or
        5-byte groups of two samples with FMT_TX10); the call writes all n_out samples.  Returns n_out."""
        k = C.c_size_t(0)
        check(self._fn("mod_stream")(self._h, self._ptr(d_bytes), self.n_bytes if in_stride is None else int(in_stride), int(n_bursts),
                                     int(start_base), int(start_step), self._ptr(d_out), int(n_out), C.byref(k), stream))
        return k.value

    def demod(self, d_in, n_in, n_bursts, d_soft, d_bits=None, d_idx=None, d_gate=None, d_rec=None, d_status=None, start_base=0, start_step=0,
              in_stride=None, idx_stride=None, gate_stride=None, soft_stride=None, bits_stride=None, status_stride=None, stream=None):
        """d_*: DeviceArray or raw device pointers.  Burst b of stream s starts at start_base + b*start_step + the uint32 at
        d_idx + s*idx_stride + b (0 without d_idx) of the n_in samples at d_in + s*in_stride, is gated by the float32 at d_gate +
        s*gate_stride + b, and writes n_bits float32 at d_soft + (s*n_bursts + b)*soft_stride, n_bytes packed bytes at d_bits +
        (s*n_bursts + b)*bits_stride, 8 float32 at d_rec + (s*n_bursts + b)*8 and an int32 at d_status + s*status_stride + b.
        in_stride defaults to n_in, soft_stride to n_bits, bits_stride to n_bytes and the other strides to n_bursts.  Returns
        n_bursts."""
        nb = int(n_bursts)
        k = C.c_size_t(0)
        check(self._fn("demod_stream")(
            self._h, self._ptr(d_in), int(n_in), int(n_in) if in_stride is None else int(in_stride), self._ptr(d_idx),
            nb if idx_stride is None else int(idx_stride), self._ptr(d_gate), nb if gate_stride is None else int(gate_stride), nb, int(start_base),
            int(start_step), self._ptr(d_soft), self.n_bits if soft_stride is None else int(soft_stride), self._ptr(d_bits),
            self.n_bytes if bits_stride is None else int(bits_stride), self._ptr(d_rec), self._ptr(d_status),
            nb if status_stride is None else int(status_stride), C.byref(k), stream))
        return k.value

    def reset(self):
        raise AttributeError("Fsk has no reset: it carries no state")

    def modulate(self, data, n_out, start_base=0, start_step=0):
        """Host convenience, computed on the GPU: data is (n_bursts, n_bytes) uint8; returns what fsk_plan returns."""
        d = np.asarray(data, dtype=np.uint8)
        d = np.ascontiguousarray(d.reshape(1, -1) if d.ndim == 1 else d)
        tx10 = self.out_fmt == _l.FMT_TX10
        nbytes = int(n_out) // 2 * 5 if tx10 else 8 * int(n_out)
        held = [DeviceArray.from_bytes(d), DeviceArray(max(1, (nbytes + 3) // 4))]
        try:
            self.mod(held[0], d.shape[0], held[1], n_out, start_base, start_step, in_stride=d.shape[1])
            raw = held[1].to_numpy().view(np.uint8)[:nbytes]
        finally:
            for x in held:
                x.free()
        return np.ascontiguousarray(raw) if tx10 else np.ascontiguousarray(raw).view(np.complex64)

    def demodulate(self, x, idx=None, gate=None, n_bursts=None, start_base=0, start_step=0):
        """Host convenience, computed on the GPU: x is (n_streams, n) complex -- or, with FMT_U8, (n_streams, 2n) uint8 (I,Q)
        pairs -- idx (uint32) and gate (float32) are (n_streams, n_bursts) or None; returns (soft (n_streams, n_bursts, n_bits)
        float32, bits (n_streams, n_bursts, n_bytes) uint8, record (n_streams, n_bursts, 8) float32, status (n_streams,
        n_bursts) int32)."""
        S, nbit, nby = self.n_streams, self.n_bits, self.n_bytes
        if idx is not None:
            idx = np.ascontiguousarray(idx, dtype=np.uint32).reshape(S, -1)
        if gate is not None:
            gate = np.ascontiguousarray(gate, dtype=np.float32).reshape(S, -1)
        nb = int(n_bursts) if n_bursts is not None else (idx.shape[1] if idx is not None else (gate.shape[1] if gate is not None else 1))
        d_in, n = self._upload_input(x)
        held = [d_in]
        try:
            d_idx = d_gate = None
            if idx is not None:
                d_idx = DeviceArray.from_numpy(idx.view(np.float32).ravel())
                held.append(d_idx)
            if gate is not None:
                d_gate = DeviceArray.from_numpy(gate.ravel())
                held.append(d_gate)
            d_soft, d_by = DeviceArray(max(1, S * nb * nbit)), DeviceArray(max(1, (S * nb * nby + 3) // 4))
            d_rec, d_st = DeviceArray(max(1, S * nb * 8)), DeviceArray(max(1, S * nb))
            held += [d_soft, d_by, d_rec, d_st]
            if nb:
                self.demod(d_in, n, nb, d_soft, d_by, d_idx, d_gate, d_rec, d_st, start_base, start_step)
            soft = d_soft.to_numpy(S * nb * nbit).reshape(S, nb, nbit)
            by = d_by.to_numpy().view(np.uint8)[:S * nb * nby].reshape(S, nb, nby)
            rec = d_rec.to_numpy(S * nb * 8).reshape(S, nb, 8)
            st = d_st.to_numpy(S * nb).view(np.int32).reshape(S, nb)
        finally:
            for d in held:
                d.free()
        return np.ascontiguousarray(soft), np.ascontiguousarray(by), np.ascontiguousarray(rec), np.ascontiguousarray(st)


def pn_bytes(m, taps, seed, n):
    """sfe_dsp_crc_pn_bytes (host only): n bytes of the additive scrambler's sequence (degree m, taps, seed), MSB first -- what
    a Crc XORs over its frames, and what makes Reed's `whiten`."""
    out = np.empty(int(n), np.uint8)
    check(_l.load().sfe_dsp_crc_pn_bytes(int(m), int(taps), int(seed), out.size, out.ctypes.data if out.size else None))
    return out


def _crc_shape(width, poly, init, reflect, xorout, pn_m, pn_taps, pn_seed, payload_bytes):
    """The nine shape arguments sfe_dsp_crc_plan and sfe_dsp_crc_create share."""
    return (int(width), int(poly), int(init), int(reflect), int(xorout), int(pn_m), int(pn_taps), int(pn_seed), int(payload_bytes))


def crc_plan(width, poly, init, reflect, xorout, pn_m=0, pn_taps=0, pn_seed=0, payload_bytes=1, data=None, verify=False, status_in=None):
    """sfe_dsp_crc_plan (host only, no GPU): validates and, without data, returns frame_bytes.  With data and not verify (the C ABI's check = 0) --
    (n_frames, >= payload_bytes) uint8 -- it returns the frames (n_frames, frame_bytes) uint8; with data and verify (check = 1) --
    (n_frames, >= frame_bytes) uint8 channel bytes -- it returns (bytes (n_frames, payload_bytes) uint8, record (n_frames, 2)
    uint32 -- the CRC computed, the CRC received -- and status (n_frames,) int32).  These are the device's bytes.
    status_in: int32 per frame or None.  Raises SfeError on arguments the block refuses."""
    head = _crc_shape(width, poly, init, reflect, xorout, pn_m, pn_taps, pn_seed, payload_bytes)
    L, Fb = _l.load(), C.c_int(0)
    check(L.sfe_dsp_crc_plan(*head, int(bool(verify)), None, 0, None, 0, None, 0, None, None, C.byref(Fb)))
    if data is None:
        return Fb.value
    d = np.asarray(data, dtype=np.uint8)
    d = np.ascontiguousarray(d.reshape(1, -1) if d.ndim == 1 else d)
    nf = d.shape[0]
    if status_in is not None:
        status_in = np.ascontiguousarray(status_in, dtype=np.int32).ravel()
        if status_in.size != nf:
            raise ValueError("crc_plan: status_in has %d entries for %d frames" % (status_in.size, nf))
    out = np.empty((nf, head[8] if verify else Fb.value), np.uint8)
    rec, st = np.empty((nf, 2), np.uint32), np.empty(nf, np.int32)
    check(L.sfe_dsp_crc_plan(*head, int(bool(verify)), d.ctypes.data if d.size else None, d.shape[1],
                              None if status_in is None else status_in.ctypes.data, nf, out.ctypes.data, out.shape[1], rec.ctypes.data,
                              st.ctypes.data, None))
    return (out, rec, st) if verify else out


class Crc(_Block):
    """Frame check (sfe_dsp_crc_*): append_stream turns payload_bytes bytes per frame into frame_bytes = payload_bytes + width / 8
    bytes -- the payload, its CRC, the whole XOR the scrambler's sequence -- in front of a Reed / Ldpc encoder, a Mod or an Fsk;
    check_stream de-scrambles channel bytes -- what a Vit, a Reed, an Ldpc or an Fsk wrote -- and writes the payload with a record
    (CRC computed, CRC received) and a status per frame.  width 0: a scrambler alone.  The device's bytes are crc_plan's."""
    _prefix = "crc"

    def __init__(self, width, poly, init, reflect, xorout, pn_m=0, pn_taps=0, pn_seed=0, payload_bytes=1, device=0):
        head = _crc_shape(width, poly, init, reflect, xorout, pn_m, pn_taps, pn_seed, payload_bytes)
        self._create(*head, device)
        self.width, self.payload_bytes, self.frame_bytes = head[0], head[8], head[8] + head[0] // 8

    def append_stream(self, d_payload, n_frames, d_frame, in_stride=None, out_stride=None, stream=None):
        """d_*: DeviceArray or raw device pointers.  Frame b reads payload_bytes bytes at d_payload + b*in_stride (default
        payload_bytes) and writes frame_bytes bytes at d_frame + b*out_stride (default frame_bytes).  Returns n_frames."""
        k = C.c_size_t(0)
        check(self._fn("append_stream")(self._h, self._ptr(d_payload), self.payload_bytes if in_stride is None else int(in_stride), int(n_frames),
                                        self._ptr(d_frame), self.frame_bytes if out_stride is None else int(out_stride), C.byref(k), stream))
        return k.value

    def check_stream(self, d_frame, n_frames, d_out=None, d_rec=None, d_status=None, d_status_in=None, in_stride=None, out_stride=None, stream=None):
        """d_*: DeviceArray or raw device pointers.  Frame b reads frame_bytes bytes at d_frame + b*in_stride (default
        frame_bytes) and, with d_status_in, the int32 at d_status_in + b; it writes payload_bytes bytes at d_out + b*out_stride
        (default payload_bytes), two words at d_rec + 2b and an int32 at d_status + b; each of the three may be None, not all.
        Returns n_frames."""
        k = C.c_size_t(0)
        check(self._fn("check_stream")(self._h, self._ptr(d_frame), self.frame_bytes if in_stride is None else int(in_stride),
                                       self._ptr(d_status_in), int(n_frames), self._ptr(d_out),
                                       self.payload_bytes if out_stride is None else int(out_stride), self._ptr(d_rec), self._ptr(d_status),
                                       C.byref(k), stream))
        return k.value

    def reset(self):
        raise AttributeError("Crc has no reset: it carries no state")

    def append(self, data):
        """Host convenience, computed on the GPU: data is (n_frames, payload_bytes) uint8; returns (n_frames, frame_bytes)."""
        d = np.asarray(data, dtype=np.uint8)
        d = np.ascontiguousarray(d.reshape(1, -1) if d.ndim == 1 else d)
        nf = d.shape[0]
        held = [DeviceArray.from_bytes(d), DeviceArray(max(1, (nf * self.frame_bytes + 3) // 4))]
        try:
            if nf:
                self.append_stream(held[0], nf, held[1], in_stride=d.shape[1])
            raw = held[1].to_numpy().view(np.uint8)[:nf * self.frame_bytes].reshape(nf, self.frame_bytes)
        finally:
            for x in held:
                x.free()
        return np.ascontiguousarray(raw)

    def check(self, frames, status_in=None):
        """Host convenience, computed on the GPU: frames is (n_frames, frame_bytes) uint8; returns what crc_plan returns."""
        d = np.asarray(frames, dtype=np.uint8)
        d = np.ascontiguousarray(d.reshape(1, -1) if d.ndim == 1 else d)
        nf, P = d.shape[0], self.payload_bytes
        held = [DeviceArray.from_bytes(d), DeviceArray(max(1, (nf * P + 3) // 4)), DeviceArray(max(1, 2 * nf)), DeviceArray(max(1, nf))]
        try:
            d_si = None
            if status_in is not None:
                d_si = DeviceArray.from_numpy(np.ascontiguousarray(status_in, dtype=np.int32).reshape(nf).view(np.float32))
                held.append(d_si)
            if nf:
                self.check_stream(held[0], nf, held[1], held[2], held[3], d_si, in_stride=d.shape[1])
            by = held[1].to_numpy().view(np.uint8)[:nf * P].reshape(nf, P)
            rec = held[2].to_numpy(2 * nf).view(np.uint32).reshape(nf, 2)
            st = held[3].to_numpy(nf).view(np.int32)
        finally:
            for x in held:
                x.free()
        return np.ascontiguousarray(by), np.ascontiguousarray(rec), np.ascontiguousarray(st)


def rs_plan(state, upsample, n_in, out_len, rate):
    """Host-only replay of one process() call's time law (sfe_dsp_rs_plan).
    state: lib.TimeState (updated in place).  Returns (rel_pos int32[], mu float32[])."""
    L = _l.load()
    cap = out_len + 1
    pos = np.zeros(cap, dtype=np.int32)
    mu = np.zeros(cap, dtype=np.float32)
    n = C.c_int(0)
    check(L.sfe_dsp_rs_plan(C.byref(state), upsample, n_in, out_len, rate, pos.ctypes.data, mu.ctypes.data, cap,
                            C.byref(n)))
    return pos[: n.value], mu[: n.value]


# ------------------------------------------------------------------ reference projection
class blkconv:
    """libdsp/blkconv.h:35-62 -- blkconv(taps, fft_len); get_blksize(); get_process_buf();
    process().  The buffer is pinned host memory owned by the object."""

    def __init__(self, taps, fft_len):
        self._fir = Fir(_f32(taps), data_complex=False, n_channels=1, block_hint=int(fft_len))
        self._buf, self._blk = self._fir.host_buffer()

    def get_blksize(self):
        return self._blk

    def get_process_buf(self):
        return self._buf

    def process(self):
        self._fir.process_block()


class _rs_class:
    _mode = None

    def __init__(self, taps, upsample, blksize):
        self._rs = Rs(taps, int(upsample), int(blksize), mode=self._mode)

    def process(self, x, out_len, rate):
        return self._rs.process(x, int(out_len), float(rate))


class resample(_rs_class):
    """libdsp/resample.h:33-61 via pydsp.i: process(in, out_len, rate) -> (n_out, out)."""
    _mode = _l.RS_RESAMPLE


class decimate(_rs_class):
    """libdsp/decimate.h:33-63 via pydsp.i."""
    _mode = _l.RS_DECIMATE
