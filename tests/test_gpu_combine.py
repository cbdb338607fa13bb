"""The polyphase synthesis filter bank on the GPU (sfe_dsp_combine_*, csrc/combine.hip) against the float64 reference
of its contract (synth.combine_reference: inverse FFT over the channels, overlap-add of g).  `-m gpu`."""
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


def _chans(M, n, n_streams, first=0):
    """(n_streams, M, n) complex64: channel k of stream s is the synth stream (s*M + k) from instant `first`."""
    return np.stack([np.stack([synth.synth_cf32(n, ch=s * M + k, first_sample=first).view(np.complex64) for k in range(M)])
                     for s in range(n_streams)])


def _taps(n_taps, M):
    return synth.lowpass_taps(n_taps, 1.0 / M) if n_taps > 1 else np.ones(1, np.float32)


def _run_calls(api, cb, X, cuts):
    """Feed (n_streams, M, n) complex64 X to handle cb in calls of the given sizes (instants); returns the device output
    as bytes (F32: (n_streams, n D) float32 pairs, TX10: the wire bytes)."""
    S, M, n = X.shape
    D = cb.interp
    n_out = n * D
    d_in = api.DeviceArray.from_numpy(X.view(np.float32))
    row_b = n_out // 2 * 5 if cb.out_tx10 else 8 * n_out
    d_out = api.DeviceArray((S * row_b + 3) // 4 + 1)
    pos = 0
    for c in cuts:
        o = pos * D
        po = d_out.ptr + (o // 2 * 5 if cb.out_tx10 else 8 * o)
        k = cb.process_stream(d_in.ptr + 8 * pos, c, po, in_stride=n, out_stride=n_out)
        assert k == c * D
        pos += c
    assert pos == n
    y = d_out.to_numpy().view(np.uint8)[: S * row_b].copy()
    d_in.free()
    d_out.free()
    return y


def _check(y, ref, tag):
    err = y.astype(np.complex128) - ref
    rms = np.sqrt(np.mean(np.abs(ref) ** 2))
    rel = np.sqrt(np.mean(np.abs(err) ** 2)) / rms
    D = tag[1]
    worst = max(np.sqrt(np.mean(np.abs(err[p::D]) ** 2)) for p in range(D)) / rms      # the worst output phase
    assert rel <= TOL and worst <= TOL, (tag, rel, worst)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("n_streams", [1, 3])
@pytest.mark.parametrize("taps_of", ["1", "8M-3", "16M", "32M"])
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("M", [4, 16, 64, 256, 1024])
def test_parity_grid(api, M, half, taps_of, n_streams):
    D = M // 2 if half else M
    n_taps = {"1": 1, "8M-3": 8 * M - 3, "16M": 16 * M, "32M": 32 * M}[taps_of]
    g = _taps(n_taps, M)
    n = 160
    X = _chans(M, n, n_streams)
    cb = api.Combiner(g, M, D, n_streams=n_streams)
    z = cb.combine(X)
    assert z.shape == (n_streams, n * D)
    for s in range(n_streams):
        _check(z[s], synth.combine_reference(X[s], g, M, D), (M, D, n_taps, s))
    cb.close()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("M", [64, 1024])
def test_cutting_the_stream_gives_the_same_bits(api, M, half):
    D = M // 2 if half else M
    g = _taps(16 * M - 5, M)
    n = 2 * 3 * 7 * 10
    X = _chans(M, n, 1)
    one = _run_calls(api, api.Combiner(g, M, D), X, [n])
    for cuts in ([1] * n, [3] * (n // 3), [7] * (n // 7), [5, 1, 33, 2, 17, 3, 7] + [1] * (n - 68)):
        got = _run_calls(api, api.Combiner(g, M, D), X, cuts)
        assert np.array_equal(got, one), (M, D, cuts[:8])


@pytest.mark.timeout(300)
@pytest.mark.parametrize("half", [False, True])
def test_reset_and_streams_are_independent(api, half):
    M = 256
    D = M // 2 if half else M
    g = _taps(8 * M - 3, M)
    n = 96
    X = _chans(M, n, 3)
    cb = api.Combiner(g, M, D, n_streams=3)
    first = cb.combine(_chans(M, n, 3, first=12345))        # something to forget
    cb.reset()
    after_reset = cb.combine(X)
    fresh = api.Combiner(g, M, D, n_streams=3).combine(X)
    assert np.array_equal(after_reset.view(np.uint32), fresh.view(np.uint32))
    assert not np.array_equal(first.view(np.uint32), fresh.view(np.uint32))
    for s in range(3):
        alone = api.Combiner(g, M, D).combine(X[s])[0]
        assert np.array_equal(alone.view(np.uint32), fresh[s].view(np.uint32)), s


@pytest.mark.timeout(300)
@pytest.mark.parametrize("M", [16, 256])
def test_channelizer_output_feeds_the_combiner_on_device(api, M):
    D = M // 2
    h = synth.lowpass_taps(16 * M + 1, 2.0 / M)
    g = synth.lowpass_taps(16 * M + 1, 1.0 / M)
    n = 160 * M
    x = synth.synth_cf32(n).view(np.complex64)
    d_x = api.DeviceArray.from_numpy(x.view(np.float32))
    n_mid = n // D
    d_mid = api.DeviceArray(2 * M * n_mid)
    d_z = api.DeviceArray(2 * n)
    assert api.Chan(h, M, D).process_stream(d_x, n, d_mid) == n_mid
    assert api.Combiner(g, M, D).process_stream(d_mid, n_mid, d_z) == n          # chan's layout read directly
    z = d_z.to_numpy().view(np.complex64).astype(np.complex128)
    for d in (d_x, d_mid, d_z):
        d.free()
    delay = 16 * M
    lo = 2 * delay
    a, b = z[lo:], x[lo - delay:n - delay].astype(np.complex128)
    gain = np.vdot(b, a) / np.vdot(b, b)
    err = np.sqrt(np.mean(np.abs(a - gain * b) ** 2)) / np.sqrt(np.mean(np.abs(gain * b) ** 2))
    assert err <= 3e-3, (M, err)
    assert abs(gain - 2.0 / M) <= 0.01 * (2.0 / M), (M, gain)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("M", [16, 256])
def test_a_channel_lands_at_its_frequency(api, M, half):
    D = M // 2 if half else M
    g = synth.lowpass_taps(16 * M, 1.0 / M)
    n = 256
    for k0 in (1, M // 2 - 1, M // 2, M - 1):
        X = np.zeros((M, n), np.complex64)
        X[k0] = 1.0
        z = api.Combiner(g, M, D).combine(X)[0].astype(np.complex128)
        w = z[64 * D:64 * D + 64 * M]                       # past the fill, whole periods of every channel
        e = np.abs(np.fft.fft(w)) ** 2
        b0 = k0 * (w.size // M)                             # the bin at k0 / M cycles per sample
        assert e[b0] >= 0.999 * e.sum(), (M, D, k0, int(np.argmax(e)), e[b0] / e.sum())


@pytest.mark.timeout(300)
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("M", [16, 256])
def test_tx10_bytes_are_the_converter_of_the_f32_output(api, L, M, half):
    D = M // 2 if half else M
    g = _taps(16 * M, M)
    n = 96
    X = _chans(M, n, 2) * np.float32(4.0 / np.sqrt(M))       # a swing across the 10-bit range
    f32 = _run_calls(api, api.Combiner(g, M, D, n_streams=2), X, [n])
    lib = L.load()
    n_out = n * D
    d_f = api.DeviceArray.from_numpy(f32.view(np.float32))
    d_b = api.DeviceArray((2 * n_out * 5 // 2 + 3) // 4 + 1)
    assert lib.sfe_dsp_tx_f32_to_10bit(d_f.ptr, d_b.ptr, 4 * n_out, None) == 0
    want = d_b.to_numpy().view(np.uint8)[: 2 * (n_out // 2 * 5)].copy()
    d_f.free()
    d_b.free()
    for cuts in ([n], [1] * n, [5, 1, 33, 2, 17, 3, 7, 28]):
        cb = api.Combiner(g, M, D, n_streams=2)
        cb.set_output_format(L.FMT_TX10)
        got = _run_calls(api, cb, X, cuts)
        assert np.array_equal(got, want), (M, D, cuts[:4])


@pytest.mark.timeout(900)
@pytest.mark.parametrize("half", [False, True])
def test_full_size_windows(api, half):
    M, n_out = 256, 1 << 28
    D = M // 2 if half else M
    g = synth.lowpass_taps(16 * M, 1.0 / M)
    n = n_out // D
    d_in = api.DeviceArray(2 * M * n)                         # channel k = synth samples [k n, (k + 1) n)
    d_in.fill_synth(synth.SEED)
    d_out = api.DeviceArray(2 * n_out)
    assert api.Combiner(g, M, D).process_stream(d_in, n, d_out) == n_out
    api.sync()
    d_in.free()
    W = 4096
    starts = sorted({*np.linspace(0, n_out - W, 31).astype(int).tolist(), (n_out // 2) // 7 * 7 + 3})   # first, last, odd
    assert len(starts) == 32 and starts[0] == 0 and starts[-1] == n_out - W
    for i0 in starts:
        first = max(0, -(-(i0 - g.size + 1) // D))
        last = (i0 + W - 1) // D
        X = np.stack([synth.synth_cf32(last + 1 - first, first_sample=k * n + first).view(np.complex64) for k in range(M)])
        ref = synth.combine_reference_direct(X, g, M, D, first, i0, W)
        got = d_out.to_numpy(2 * W, offset=2 * i0).view(np.complex64)
        rel = synth.rel_rms(got.view(np.float32), np.ascontiguousarray(ref).view(np.float64))
        assert rel <= TOL, (D, i0, rel)
    d_out.free()


@pytest.mark.timeout(300)
def test_refusals_launch_nothing(api, L):
    M, D = 64, 32
    g = _taps(8 * M, M)
    n = 64
    X = _chans(M, n, 1)
    cb = api.Combiner(g, M, D)
    d_in = api.DeviceArray.from_numpy(X.view(np.float32))
    sentinel = np.full(2 * n * D, 1234.5, np.float32)
    d_out = api.DeviceArray.from_numpy(sentinel)
    lib = L.load()
    k = C.c_size_t(7)

    def call(pi, n_in, in_stride, po, out_stride):
        return lib.sfe_dsp_combine_process_stream(cb._h, pi, n_in, in_stride, po, out_stride, C.byref(k), None)

    assert call(d_in.ptr, n, n - 1, d_out.ptr, n * D) == L.SFE_EINVAL            # in_stride < n_in
    assert call(d_in.ptr, n, n, d_out.ptr, n * D - 1) == L.SFE_ERANGE            # out_stride < n_out
    assert call(d_in.ptr, n, n, d_in.ptr + 8 * 16, n * D) == L.SFE_EINVAL        # output overlaps input
    assert call(d_in.ptr + 4, n, n, d_out.ptr, n * D) == L.SFE_EINVAL            # misaligned input
    assert call(d_in.ptr, n, n, d_out.ptr + 4, n * D) == L.SFE_EINVAL            # misaligned cf32 output
    cb.set_output_format(L.FMT_TX10)
    assert call(d_in.ptr, n, n, d_out.ptr, n * D + 1) == L.SFE_EINVAL            # odd out_stride under TX10
    cb.set_output_format(L.FMT_F32)
    assert k.value == 0
    api.sync()
    assert np.array_equal(d_out.to_numpy(), sentinel)
    assert np.array_equal(d_in.to_numpy(), X.view(np.float32).ravel())
    # nothing advanced either: the next good call is a fresh handle's
    assert cb.process_stream(d_in, n, d_out) == n * D
    fresh = api.Combiner(g, M, D).combine(X)
    assert np.array_equal(d_out.to_numpy().view(np.uint32), fresh.view(np.float32).ravel().view(np.uint32))
