"""The digital down-converter bank on the GPU (sfe_dsp_ddc_*, csrc/ddc.hip) against the float64 references of its contract
(synth.ddc_reference: mix with the exact integer phase, FFT-convolve, decimate, tuning by tuning), the channelizer, and
the library composition a user has without it.  `-m gpu`."""
import ctypes as C

import numpy as np
import pytest

from simplefe_amd import synth

pytestmark = pytest.mark.gpu
TOL = 1e-5


@pytest.fixture(scope="module")
def api():
    from simplefe_amd import api as a
    return a


@pytest.fixture(scope="module")
def L():
    from simplefe_amd import lib
    return lib


def _streams(n, n_streams, first=0):
    return np.stack([synth.synth_cf32(n, ch=s, first_sample=first).view(np.complex64) for s in range(n_streams)])


def _real_streams(n, n_streams, first=0):
    return np.stack([synth.synth_f32(n, ch=s, first=first) for s in range(n_streams)])


def _taps(n_taps, D):
    return synth.lowpass_taps(n_taps, 0.5 / D) if n_taps > 1 else np.ones(1, np.float32)


def _freqs(K, seed=0):
    """K frequencies over [-0.5, 0.5], both ends and 0 among them when K >= 3."""
    f = np.random.default_rng(seed).uniform(-0.5, 0.5, K)
    if K >= 3:
        f[:3] = (0.5, -0.5, 0.0)
    return f


def _rel(got, ref):
    """rel-RMS of each (tuning) row against the reference's RMS over the row; the worst row."""
    err = got.astype(np.complex128) - ref
    rms = np.sqrt(np.mean(np.abs(ref) ** 2, axis=-1))
    return float(np.max(np.sqrt(np.mean(np.abs(err) ** 2, axis=-1)) / np.maximum(rms, 1e-30)))


def _run_calls(api, dd, x, cuts):
    """Feed (n_streams, n) complex64 x to handle dd in calls of the given sizes; returns (n_streams, K, n_out) as float32
    pairs (bit comparisons)."""
    S, n = x.shape
    K, D = dd.n_tunings, dd.decim
    n_out = n // D
    d_in = api.DeviceArray.from_numpy(x.view(np.float32))
    d_out = api.DeviceArray(S * K * n_out * 2)
    pos = 0
    for c in cuts:
        k = dd.process_stream(d_in.ptr + 8 * pos, c, d_out.ptr + 8 * (pos // D), in_stride=n, out_stride=n_out)
        assert k == c // D
        pos += c
    assert pos == n
    y = d_out.to_numpy().reshape(S, K, n_out, 2)
    d_in.free()
    d_out.free()
    return y


def _grid():
    out = []
    for D in (1, 3, 8, 10, 64, 500, 1024):
        for taps_of in ("1", "8D-3", "16D"):
            n_taps = {"1": 1, "8D-3": 8 * D - 3, "16D": 16 * D}[taps_of]
            if n_taps > 8192 or -(-n_taps // D) > 64 or n_taps < 1:
                continue
            out.append((D, n_taps))
    return sorted(set(out))


@pytest.mark.timeout(900)
@pytest.mark.parametrize("fmt", ["cf32", "u8", "real"])
@pytest.mark.parametrize("D, n_taps", _grid())
def test_parity_grid(api, L, D, n_taps, fmt):
    h = _taps(n_taps, D)
    n = D * max(64, -(-4 * n_taps // D))
    for K in (1, 3, 64):
        f = _freqs(K, seed=D + K)
        incs = synth.ddc_incs(f)
        for S in (1, 3):
            if fmt == "real":
                x = _real_streams(n, S)
                dd = api.Ddc(h, D, f, data_complex=False, n_streams=S)
                y = dd.downconvert(x)
                xr = x.astype(np.float64)
            elif fmt == "u8":
                b = np.random.default_rng(D * 7 + S).integers(0, 256, size=(S, 2 * n), dtype=np.uint8)
                dd = api.Ddc(h, D, f, n_streams=S)
                dd.set_input_format(L.FMT_U8)
                y = dd.downconvert(b)
                v = (b.astype(np.float32) - np.float32(128.0)) * np.float32(1.0 / 127.0)
                xr = v[:, 0::2].astype(np.float64) + 1j * v[:, 1::2].astype(np.float64)
            else:
                x = _streams(n, S)
                dd = api.Ddc(h, D, f, n_streams=S)
                y = dd.downconvert(x)
                xr = x
            dd.close()
            assert y.shape == (S, K, n // D)
            for s in range(S):
                rel = _rel(y[s], synth.ddc_reference(xr[s], h, D, incs))
                assert rel <= TOL, (D, n_taps, fmt, K, S, s, rel)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("D", [1, 10, 64, 1000])
def test_cutting_the_stream_gives_the_same_bits(api, D):
    n_taps = min(8192, 16 * D - 5) if D > 1 else 37
    h = _taps(n_taps, D)
    f = _freqs(5, seed=D)
    n = D * 42 * 3 * 7 * (1 if D >= 64 else 4)
    x = _streams(n, 2)
    one = _run_calls(api, api.Ddc(h, D, f, n_streams=2), x, [n])
    nb = n // D
    for cuts in ([D] * nb, [3 * D] * (nb // 3), [7 * D] * (nb // 7), [5 * D, D, 33 * D, 2 * D, 17 * D, 3 * D, 7 * D] + [D] * (nb - 68)):
        got = _run_calls(api, api.Ddc(h, D, f, n_streams=2), x, cuts)
        assert np.array_equal(got.view(np.uint32), one.view(np.uint32)), (D, cuts[:8])


@pytest.mark.timeout(300)
@pytest.mark.parametrize("data_complex", [True, False])
def test_reset_and_streams_are_independent(api, data_complex):
    D, K = 10, 3
    h = _taps(8 * D - 3, D)
    f = _freqs(K, seed=1)
    n = 400 * D
    mk = _streams if data_complex else _real_streams
    x = mk(n, 3)
    dd = api.Ddc(h, D, f, data_complex=data_complex, n_streams=3)
    first = dd.downconvert(mk(n, 3, first=12345))          # something to forget: history and the counter
    dd.reset()
    after_reset = dd.downconvert(x)
    fresh = api.Ddc(h, D, f, data_complex=data_complex, n_streams=3).downconvert(x)
    assert np.array_equal(after_reset.view(np.uint32), fresh.view(np.uint32))
    assert not np.array_equal(first.view(np.uint32), fresh.view(np.uint32))
    for s in range(3):
        alone = api.Ddc(h, D, f, data_complex=data_complex).downconvert(x[s])[0]
        assert np.array_equal(alone.view(np.uint32), fresh[s].view(np.uint32)), s


@pytest.mark.timeout(300)
@pytest.mark.parametrize("offset", [0, 2, 6])
@pytest.mark.parametrize("D, K", [(10, 1), (64, 8), (500, 3)])
def test_u8_input_equals_converted_cf32(api, L, D, K, offset):
    h = _taps(16 * D if D <= 500 else 8192, D)
    f = _freqs(K, seed=offset)
    n = 96 * D
    rng = np.random.default_rng(D + offset)
    b = rng.integers(0, 256, size=2 * n, dtype=np.uint8)
    lib = L.load()
    # cf32 path: the library's own converter over an aligned copy of the bytes
    d_b = api.DeviceArray.from_bytes(b)
    d_f = api.DeviceArray(2 * n)
    assert lib.sfe_dsp_rx_u8_to_f32(d_b.ptr, d_f.ptr, 2 * n, None) == 0
    d_ref = api.DeviceArray(2 * K * (n // D))
    assert api.Ddc(h, D, f).process_stream(d_f, n, d_ref) == n // D
    want = d_ref.to_numpy()
    # u8 path: the same bytes at `offset` bytes past a 16-byte boundary, fed in two calls
    d_u = api.DeviceArray((2 * n + offset) // 4 + 8)
    assert d_u.ptr % 16 == 0
    assert lib.sfe_dsp_memcpy_h2d(d_u.ptr + offset, b.ctypes.data, 2 * n, None) == 0
    dd = api.Ddc(h, D, f)
    dd.set_input_format(L.FMT_U8)
    d_out = api.DeviceArray(2 * K * (n // D))
    cut = 17 * D
    k1 = dd.process_stream(d_u.ptr + offset, cut, d_out.ptr, out_stride=n // D)
    k2 = dd.process_stream(d_u.ptr + offset + 2 * cut, n - cut, d_out.ptr + 8 * k1, out_stride=n // D)
    assert k1 + k2 == n // D
    assert np.array_equal(d_out.to_numpy().view(np.uint32), want.view(np.uint32)), (D, K, offset)
    # the format may change between calls: cf32 after u8 continues the same stream
    dd2 = api.Ddc(h, D, f)
    dd2.set_input_format(L.FMT_U8)
    d_o2 = api.DeviceArray(2 * K * (n // D))
    dd2.process_stream(d_u.ptr + offset, cut, d_o2.ptr, out_stride=n // D)
    dd2.set_input_format(L.FMT_F32)
    dd2.process_stream(d_f.ptr + 8 * cut, n - cut, d_o2.ptr + 8 * k1, out_stride=n // D)
    assert np.array_equal(d_o2.to_numpy().view(np.uint32), want.view(np.uint32))


@pytest.mark.timeout(300)
@pytest.mark.parametrize("M", [4, 16, 64])
@pytest.mark.parametrize("half", [False, True])
def test_agrees_with_the_channelizer(api, M, half):
    D = M // 2 if half else M
    h = synth.lowpass_taps(16 * M, 1.0 / M)
    f = [(k / M + 0.5) % 1.0 - 0.5 for k in range(M)]          # k/M mapped into [-0.5, 0.5): the same increments
    assert synth.ddc_incs(f) == [(k << 32) // M for k in range(M)]
    x = _streams(256 * M, 1)
    want = api.Chan(h, M, D).channelize(x)[0]
    got = api.Ddc(h, D, f).downconvert(x)[0]
    assert _rel(got, want.astype(np.complex128)) <= TOL, (M, D)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("data_complex", [True, False])
@pytest.mark.parametrize("D", [10, 100])
def test_agrees_with_the_library_composition(api, D, data_complex):
    """A complex-tap FIR at the full rate per tuning, every D-th output, the lead factor: what a user composes today."""
    h = _taps(16 * D, D)
    f = _freqs(3, seed=D)
    incs = synth.ddc_incs(f)
    n = 512 * D
    x = _streams(n, 1)[0] if data_complex else _real_streams(n, 1)[0]
    got = api.Ddc(h, D, f, data_complex=data_complex).downconvert(x)[0]
    m = np.arange(n // D)
    for k, inc in enumerate(incs):
        g = (h.astype(np.float64) * np.conj(synth._ddc_phase(np.arange(h.size), inc))).astype(np.complex64)
        fir = api.Fir(g, data_complex=data_complex)
        xin = x.view(np.float32) if data_complex else x
        full = fir.filter(xin).view(np.complex64).ravel()
        fir.close()
        composed = full[m * D].astype(np.complex128) * synth._ddc_phase(m * D, inc)
        assert _rel(got[k][None], composed[None]) <= TOL, (D, k, data_complex)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("D", [10, 64])
def test_a_tone_comes_out_at_dc(api, D):
    h = synth.lowpass_taps(16 * D, 0.5 / D)
    n = 400 * D
    f0 = 0.1234567
    x = np.exp(2j * np.pi * f0 * np.arange(n)).astype(np.complex64)
    # tuned at f0: DC of sum(h) after the filter fills; a stopband away: below the filter's stopband level
    y = api.Ddc(h, D, [f0, f0 + 4.0 / D if f0 + 4.0 / D <= 0.5 else f0 - 4.0 / D]).downconvert(x)[0][:, 20:]
    dc = float(np.sum(h.astype(np.float64)))
    assert np.max(np.abs(y[0] - dc)) <= 1e-4 * abs(dc), np.max(np.abs(y[0] - dc))
    H = np.abs(np.fft.fft(h.astype(np.float64), 1 << 16))
    fr = np.fft.fftfreq(1 << 16)
    stop = H[np.abs(fr) >= 3.0 / D].max()
    assert np.max(np.abs(y[1])) <= 1.01 * stop + 1e-5 * abs(dc), (np.max(np.abs(y[1])), stop)


@pytest.mark.timeout(300)
def test_set_freqs(api):
    D, K = 10, 4
    h = _taps(8 * D - 3, D)
    f_old, f_new = _freqs(K, seed=3), _freqs(K, seed=4)
    n = 300 * D
    x = _streams(n, 1)
    cut = 120 * D
    dd = api.Ddc(h, D, f_old)
    d_in = api.DeviceArray.from_numpy(x.view(np.float32))
    d_out = api.DeviceArray(2 * K * (n // D))
    n_out = n // D
    # the first call is enqueued and not waited for: set_freqs must not change what it computes
    assert dd.process_stream(d_in.ptr, cut, d_out.ptr, in_stride=n, out_stride=n_out) == cut // D
    dd.set_freqs(f_new)
    assert dd.process_stream(d_in.ptr + 8 * cut, n - cut, d_out.ptr + 8 * (cut // D), in_stride=n, out_stride=n_out) == (n - cut) // D
    got = d_out.to_numpy().reshape(K, n_out, 2)
    old = api.Ddc(h, D, f_old).downconvert(x)[0].view(np.float32).reshape(K, n_out, 2)
    new = api.Ddc(h, D, f_new).downconvert(x)[0].view(np.float32).reshape(K, n_out, 2)
    assert np.array_equal(got[:, : cut // D].view(np.uint32), old[:, : cut // D].view(np.uint32))
    assert np.array_equal(got[:, cut // D:].view(np.uint32), new[:, cut // D:].view(np.uint32))
    # a retune to a bad frequency is refused and changes nothing
    from simplefe_amd import lib
    with pytest.raises(lib.SfeError):
        dd.set_freqs([0.1, 0.2, 0.7, 0.0])
    d_in.free()
    d_out.free()


def _u8_window(first_sample, count, period=None):
    """Samples [first_sample, first_sample + count) of the u8 stream that is the byte image of the synth_fill float
    stream (seed SEED, channel 0) -- repeated every `period` samples when given -- converted as the device does."""
    if period is not None:
        idx = (first_sample + np.arange(count, dtype=np.int64)) % period
        lo, hi = int(idx.min()), int(idx.max()) + 1
        if (idx[-1] - idx[0]) == count - 1:                # no wrap inside the window
            return _u8_window(int(idx[0]), count)
        a = _u8_window(int(idx[0]), period - int(idx[0]))
        b = _u8_window(0, count - a.size)
        assert lo >= 0 and hi <= period
        return np.concatenate([a, b])
    f0 = (2 * first_sample) // 4
    nf = (2 * (first_sample + count) + 3) // 4 - f0
    by = synth.synth_f32(nf, first=f0).view(np.uint8)[2 * first_sample - 4 * f0:][: 2 * count]
    v = (by.astype(np.float32) - np.float32(128.0)) * np.float32(1.0 / 127.0)
    return v[0::2].astype(np.float64) + 1j * v[1::2].astype(np.float64)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("fmt", ["cf32", "u8"])
def test_full_size_windows(api, L, fmt):
    """2^28 samples in two calls (the seam at a multiple of D that is not a power of two), windows against the direct
    reference."""
    n, D, K = 1 << 28, 100, 3
    n1 = (n // 2) // D * D
    n_use = n // D * D
    h = synth.lowpass_taps(16 * D, 0.5 / D)
    f = [0.3141592653589793, -0.4567, 0.0123]
    incs = synth.ddc_incs(f)
    d_in = api.DeviceArray(2 * n) if fmt == "cf32" else api.DeviceArray(n // 2)
    d_in.fill_synth(synth.SEED)
    n_out = n_use // D
    d_out = api.DeviceArray(2 * K * n_out)
    dd = api.Ddc(h, D, f)
    isz = 8
    if fmt == "u8":
        dd.set_input_format(L.FMT_U8)
        isz = 2
    assert dd.process_stream(d_in.ptr, n1, d_out.ptr, out_stride=n_out) == n1 // D
    assert dd.process_stream(d_in.ptr + isz * n1, n_use - n1, d_out.ptr + 8 * (n1 // D), out_stride=n_out) == (n_use - n1) // D
    api.sync()
    d_in.free()
    W = 2048
    starts = sorted({*np.linspace(0, n_out - W, 15).astype(int).tolist(), n1 // D - W // 2})    # the seam inside one window
    for m0 in starts:
        a = max(0, m0 * D - (h.size - 1))
        cnt = (m0 + W - 1) * D + 1 - a
        xw = synth.synth_cf32(cnt, first_sample=a).view(np.complex64) if fmt == "cf32" else _u8_window(a, cnt)
        ref = synth.ddc_reference_direct(xw, h, D, incs, a, m0, W)
        got = np.stack([d_out.to_numpy(2 * W, offset=2 * (k * n_out + m0)).view(np.complex64) for k in range(K)])
        assert _rel(got, ref) <= TOL, (fmt, m0)
    d_out.free()


@pytest.mark.timeout(900)
def test_sample_counter_past_2_to_the_32(api, L):
    """One 2^28-sample u8 buffer fed 17 times: the last call's samples are 16 2^28 .. 17 2^28 - 1 > 2^32.  Any 32-bit
    index or phase product on the host or in the kernel shows in its windows."""
    n, D, K, reps = 1 << 28, 64, 3, 17
    h = synth.lowpass_taps(16 * D - 3, 0.5 / D)
    f = [0.3141592653589793, -0.2718281828, 0.4999]
    incs = synth.ddc_incs(f)
    d_in = api.DeviceArray(n // 2)
    d_in.fill_synth(synth.SEED)
    n_out = n // D
    d_out = api.DeviceArray(2 * K * n_out)
    dd = api.Ddc(h, D, f)
    dd.set_input_format(L.FMT_U8)
    for _ in range(reps):
        assert dd.process_stream(d_in, n, d_out) == n_out
    api.sync()
    d_in.free()
    W = 1024
    base = (reps - 1) * n                       # absolute index of the last call's first sample
    for m0 in (0, 5, n_out // 3, n_out - W):
        ma = base // D + m0
        a = ma * D - (h.size - 1)
        cnt = (ma + W - 1) * D + 1 - a
        xw = _u8_window(a, cnt, period=n)
        ref = synth.ddc_reference_direct(xw, h, D, incs, a, ma, W)
        got = np.stack([d_out.to_numpy(2 * W, offset=2 * (k * n_out + m0)).view(np.complex64) for k in range(K)])
        assert _rel(got, ref) <= TOL, m0
    d_out.free()


@pytest.mark.timeout(300)
def test_refusals_launch_nothing(api, L):
    D, K = 10, 3
    h = _taps(8 * D, D)
    f = _freqs(K, seed=9)
    n = 64 * D
    x = _streams(n, 1)
    dd = api.Ddc(h, D, f)
    d_in = api.DeviceArray.from_numpy(x.view(np.float32))
    sentinel = np.full(2 * K * (n // D), 1234.5, np.float32)
    d_out = api.DeviceArray.from_numpy(sentinel)
    lib = L.load()
    k = C.c_size_t(7)

    def call(pi, n_in, in_stride, po, out_stride):
        return lib.sfe_dsp_ddc_process_stream(dd._h, pi, n_in, in_stride, po, out_stride, C.byref(k), None)

    assert call(d_in.ptr, n - 1, n, d_out.ptr, n // D) == L.SFE_EINVAL            # n_in not a multiple of D
    assert call(d_in.ptr, n, n, d_out.ptr, n // D - 1) == L.SFE_ERANGE            # out_stride < n_out
    assert call(d_in.ptr, n, n, d_in.ptr + 8 * 16, n // D) == L.SFE_EINVAL        # output overlaps input
    assert call(d_in.ptr + 4, n, n, d_out.ptr, n // D) == L.SFE_EINVAL            # misaligned cf32 input
    assert call(d_in.ptr, n, n, d_out.ptr + 4, n // D) == L.SFE_EINVAL            # misaligned output
    assert call(d_in.ptr, (1 << 31) // D * D + D, n, d_out.ptr, 1 << 31) == L.SFE_EINVAL   # n_in >= 2^31
    assert k.value == 0
    # two streams with in_stride < n_in
    dd2 = api.Ddc(h, D, f, n_streams=2)
    assert lib.sfe_dsp_ddc_process_stream(dd2._h, d_in.ptr, n // 2, n // 2 - D, d_out.ptr, n // D, C.byref(k), None) == L.SFE_EINVAL
    # real handles take no u8
    dr = api.Ddc(h, D, f, data_complex=False)
    with pytest.raises(L.SfeError):
        dr.set_input_format(L.FMT_U8)
    api.sync()
    assert np.array_equal(d_out.to_numpy(), sentinel)
    assert np.array_equal(d_in.to_numpy(), x.view(np.float32).ravel())
    # nothing advanced either: the next good call is a fresh handle's
    assert dd.process_stream(d_in, n, d_out) == n // D
    fresh = api.Ddc(h, D, f).downconvert(x)
    assert np.array_equal(d_out.to_numpy().view(np.uint32), fresh.view(np.float32).ravel().view(np.uint32))


@pytest.mark.timeout(300)
def test_graph_capture_is_refused(api, L):
    """The sample counter lives on the host: a call on a capturing stream is SFE_ESTATE and enqueues nothing."""
    hip = C.CDLL("libamdhip64.so")
    for name, args in (("hipStreamCreate", [C.POINTER(C.c_void_p)]), ("hipStreamBeginCapture", [C.c_void_p, C.c_int]),
                       ("hipStreamEndCapture", [C.c_void_p, C.POINTER(C.c_void_p)]), ("hipGraphDestroy", [C.c_void_p]),
                       ("hipStreamDestroy", [C.c_void_p])):
        fn = getattr(hip, name)
        fn.argtypes, fn.restype = args, C.c_int
    D, K = 10, 2
    h = _taps(8 * D, D)
    f = _freqs(K)
    dd = api.Ddc(h, D, f)
    n = 64 * D
    x = _streams(n, 1)
    d_in = api.DeviceArray.from_numpy(x.view(np.float32))
    sentinel = np.full(2 * K * (n // D), 7.0, np.float32)
    d_out = api.DeviceArray.from_numpy(sentinel)
    k = C.c_size_t(5)
    s = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(s)) == 0
    assert hip.hipStreamBeginCapture(s, 2) == 0            # relaxed mode: the refused call launches nothing
    try:
        rc = L.load().sfe_dsp_ddc_process_stream(dd._h, d_in.ptr, n, n, d_out.ptr, n // D, C.byref(k), s.value)
    finally:
        g = C.c_void_p()
        hip.hipStreamEndCapture(s, C.byref(g))
    if g.value:
        hip.hipGraphDestroy(g)
    hip.hipStreamDestroy(s)
    assert rc == L.SFE_ESTATE and k.value == 0
    api.sync()
    assert np.array_equal(d_out.to_numpy(), sentinel)
    assert dd.process_stream(d_in, n, d_out) == n // D          # and the counter did not move
    assert np.array_equal(d_out.to_numpy().view(np.uint32), api.Ddc(h, D, f).downconvert(x).view(np.float32).ravel().view(np.uint32))
