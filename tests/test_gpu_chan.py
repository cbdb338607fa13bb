"""The polyphase channelizer on the GPU (sfe_dsp_chan_*, csrc/chan.hip) against the float64 reference of its contract
(synth.chan_reference: mix, FFT-convolve, decimate, channel by channel).  `-m gpu`."""
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


def _taps(n_taps, M):
    return synth.lowpass_taps(n_taps, 1.0 / M) if n_taps > 1 else np.ones(1, np.float32)


def _run_calls(api, ch, x, cuts):
    """Feed (n_streams, n) complex64 x to handle ch in calls of the given sizes; returns (n_streams, M, n_out) as float32
    pairs (bit comparisons)."""
    S, n = x.shape
    M, D = ch.n_chans, ch.decim
    n_out = n // D
    d_in = api.DeviceArray.from_numpy(x.view(np.float32))
    d_out = api.DeviceArray(S * M * n_out * 2)
    pos = 0
    for c in cuts:
        k = ch.process_stream(d_in.ptr + 8 * pos, c, d_out.ptr + 8 * (pos // D), in_stride=n, out_stride=n_out)
        assert k == c // D
        pos += c
    assert pos == n
    y = d_out.to_numpy().reshape(S, M, n_out, 2)
    d_in.free()
    d_out.free()
    return y


@pytest.mark.timeout(300)
@pytest.mark.parametrize("n_streams", [1, 3])
@pytest.mark.parametrize("taps_of", ["1", "8M-3", "16M"])
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("M", [4, 16, 64, 256, 1024])
def test_parity_grid(api, M, half, taps_of, n_streams):
    D = M // 2 if half else M
    n_taps = {"1": 1, "8M-3": 8 * M - 3, "16M": 16 * M}[taps_of]
    h = _taps(n_taps, M)
    n = 64 * M
    x = _streams(n, n_streams)
    ch = api.Chan(h, M, D, n_streams=n_streams)
    y = ch.channelize(x)
    assert y.shape == (n_streams, M, n // D)
    for s in range(n_streams):
        ref = synth.chan_reference(x[s], h, M, D)
        err = y[s].astype(np.complex128) - ref
        rms = np.sqrt(np.mean(np.abs(ref) ** 2))
        rel = np.sqrt(np.mean(np.abs(err) ** 2)) / rms
        worst = np.sqrt(np.mean(np.abs(err) ** 2, axis=1)).max() / rms
        assert rel <= TOL and worst <= TOL, (M, D, n_taps, s, rel, worst)
    ch.close()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("M", [64, 1024])
def test_cutting_the_stream_gives_the_same_bits(api, M, half):
    D = M // 2 if half else M
    h = _taps(16 * M - 5, M)
    n = 42 * 3 * 7 * D
    x = _streams(n, 1)
    one = _run_calls(api, api.Chan(h, M, D), x, [n])
    for cuts in ([D] * (n // D), [3 * D] * (n // (3 * D)), [7 * D] * (n // (7 * D)),
                 [5 * D, D, 33 * D, 2 * D, 17 * D, 3 * D, 7 * D] + [D] * (n // D - 68)):
        got = _run_calls(api, api.Chan(h, M, D), x, cuts)
        assert np.array_equal(got.view(np.uint32), one.view(np.uint32)), (M, D, cuts[:8])


@pytest.mark.timeout(300)
@pytest.mark.parametrize("half", [False, True])
def test_reset_and_streams_are_independent(api, half):
    M = 256
    D = M // 2 if half else M
    h = _taps(8 * M - 3, M)
    n = 40 * M
    x = _streams(n, 3)
    ch = api.Chan(h, M, D, n_streams=3)
    first = ch.channelize(_streams(n, 3, first=12345))      # something to forget
    ch.reset()
    after_reset = ch.channelize(x)
    fresh = api.Chan(h, M, D, n_streams=3).channelize(x)
    assert np.array_equal(after_reset.view(np.uint32), fresh.view(np.uint32))
    assert not np.array_equal(first.view(np.uint32), fresh.view(np.uint32))
    for s in range(3):
        alone = api.Chan(h, M, D).channelize(x[s])[0]
        assert np.array_equal(alone.view(np.uint32), fresh[s].view(np.uint32)), s


@pytest.mark.timeout(300)
@pytest.mark.parametrize("offset", [0, 2, 6])
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("M", [16, 256])
def test_u8_input_equals_converted_cf32(api, L, M, half, offset):
    D = M // 2 if half else M
    h = _taps(16 * M, M)
    n = 48 * M
    rng = np.random.default_rng(M + offset)
    b = rng.integers(0, 256, size=2 * n, dtype=np.uint8)
    lib = L.load()
    # cf32 path: the library's own converter over an aligned copy of the bytes
    d_b = api.DeviceArray.from_bytes(b)
    d_f = api.DeviceArray(2 * n)
    assert lib.sfe_dsp_rx_u8_to_f32(d_b.ptr, d_f.ptr, 2 * n, None) == 0
    ref_ch = api.Chan(h, M, D)
    d_ref = api.DeviceArray(2 * M * (n // D))
    assert ref_ch.process_stream(d_f, n, d_ref) == n // D
    want = d_ref.to_numpy()
    # u8 path: the same bytes at `offset` bytes past a 16-byte boundary, fed in two calls
    d_u = api.DeviceArray((2 * n + offset) // 4 + 8)
    assert d_u.ptr % 16 == 0
    assert lib.sfe_dsp_memcpy_h2d(d_u.ptr + offset, b.ctypes.data, 2 * n, None) == 0
    ch = api.Chan(h, M, D)
    ch.set_input_format(L.FMT_U8)
    d_out = api.DeviceArray(2 * M * (n // D))
    cut = 17 * D
    k1 = ch.process_stream(d_u.ptr + offset, cut, d_out.ptr, out_stride=n // D)
    k2 = ch.process_stream(d_u.ptr + offset + 2 * cut, n - cut, d_out.ptr + 8 * k1, out_stride=n // D)
    assert k1 + k2 == n // D
    got = d_out.to_numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (M, D, offset)
    # and channelize() with u8 bytes
    ch2 = api.Chan(h, M, D)
    ch2.set_input_format(L.FMT_U8)
    assert np.array_equal(ch2.channelize(b)[0].view(np.float32).ravel().view(np.uint32), want.view(np.uint32))


@pytest.mark.timeout(300)
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("M", [16, 256])
def test_a_tone_lands_in_its_channel(api, M, half):
    D = M // 2 if half else M
    h = synth.lowpass_taps(16 * M, 1.0 / M)
    n = 256 * M
    for k0 in (1, M // 2 - 1, M // 2, M - 1):
        f = (k0 + 0.1) / M
        x = np.exp(2j * np.pi * f * np.arange(n)).astype(np.complex64)
        y = api.Chan(h, M, D).channelize(x)[0][:, 40:]          # past the filter's fill
        e = np.sum(np.abs(y.astype(np.complex128)) ** 2, axis=1)
        assert int(np.argmax(e)) == k0 and e[k0] >= 0.999 * e.sum(), (M, D, k0, int(np.argmax(e)), e[k0] / e.sum())


def _u8_window(first_sample, count):
    """Bytes (I,Q) of samples [first_sample, first_sample + count) of the u8 stream that is the byte image of the
    synth_fill float stream (seed SEED, channel 0), converted as the device does."""
    f0 = (2 * first_sample) // 4               # the floats covering those bytes
    nf = (2 * (first_sample + count) + 3) // 4 - f0
    by = synth.synth_f32(nf, first=f0).view(np.uint8)[2 * first_sample - 4 * f0:][: 2 * count]
    v = (by.astype(np.float32) - np.float32(128.0)) * np.float32(1.0 / 127.0)
    return v[0::2].astype(np.float64) + 1j * v[1::2].astype(np.float64)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("fmt", ["cf32", "u8"])
@pytest.mark.parametrize("half", [False, True])
def test_full_size_windows(api, L, half, fmt):
    M, n = 256, 1 << 28
    D = M // 2 if half else M
    h = synth.lowpass_taps(16 * M, 1.0 / M)
    n_out = n // D
    if fmt == "cf32":
        d_in = api.DeviceArray(2 * n)
        d_in.fill_synth(synth.SEED)
    else:
        d_in = api.DeviceArray(n // 2)            # 2n bytes: the byte image of n/2 synth floats
        d_in.fill_synth(synth.SEED)
    d_out = api.DeviceArray(2 * M * n_out)
    ch = api.Chan(h, M, D)
    if fmt == "u8":
        ch.set_input_format(L.FMT_U8)
    assert ch.process_stream(d_in, n, d_out) == n_out
    api.sync()
    d_in.free()
    W = 4096
    starts = sorted({*np.linspace(0, n_out - W, 31).astype(int).tolist(), (n_out // 2) // 7 * 7 + 3})   # first, last, odd
    assert len(starts) == 32 and starts[0] == 0 and starts[-1] == n_out - W
    Lh = h.size
    for m0 in starts:
        a = max(0, m0 * D - (Lh - 1))
        cnt = (m0 + W - 1) * D + 1 - a
        xw = synth.synth_cf32(cnt, first_sample=a).view(np.complex64) if fmt == "cf32" else _u8_window(a, cnt)
        ref = synth.chan_reference_direct(xw, h, M, D, a, m0, W)
        got = np.stack([d_out.to_numpy(2 * W, offset=2 * (k * n_out + m0)).view(np.complex64) for k in range(M)])
        rel = synth.rel_rms(got.view(np.float32), np.ascontiguousarray(ref).view(np.float64))
        assert rel <= TOL, (D, fmt, m0, rel)
    d_out.free()


@pytest.mark.timeout(300)
def test_refusals_launch_nothing(api, L):
    M, D = 64, 32
    h = _taps(8 * M, M)
    n = 32 * M
    x = _streams(n, 1)
    ch = api.Chan(h, M, D)
    d_in = api.DeviceArray.from_numpy(x.view(np.float32))
    sentinel = np.full(2 * M * (n // D), 1234.5, np.float32)
    d_out = api.DeviceArray.from_numpy(sentinel)
    lib = L.load()
    k = C.c_size_t(7)

    def call(pi, n_in, in_stride, po, out_stride):
        return lib.sfe_dsp_chan_process_stream(ch._h, pi, n_in, in_stride, po, out_stride, C.byref(k), None)

    assert call(d_in.ptr, n - 1, n, d_out.ptr, n // D) == L.SFE_EINVAL            # n_in not a multiple of D
    assert call(d_in.ptr, n, n, d_out.ptr, n // D - 1) == L.SFE_ERANGE            # out_stride < n_out
    assert call(d_in.ptr, n, n, d_in.ptr + 8 * 16, n // D) == L.SFE_EINVAL        # output overlaps input
    assert call(d_in.ptr + 4, n, n, d_out.ptr, n // D) == L.SFE_EINVAL            # misaligned cf32 input
    assert k.value == 0
    api.sync()
    assert np.array_equal(d_out.to_numpy(), sentinel)
    assert np.array_equal(d_in.to_numpy(), x.view(np.float32).ravel())
    # nothing advanced either: the next good call is a fresh handle's
    assert ch.process_stream(d_in, n, d_out) == n // D
    fresh = api.Chan(h, M, D).channelize(x)
    assert np.array_equal(d_out.to_numpy().view(np.uint32), fresh.view(np.float32).ravel().view(np.uint32))
