"""The streaming biquad-cascade IIR filter on the GPU (sfe_dsp_iir_*, csrc/iir.hip) against the float64 reference of
its law (synth.iir_reference), and the parts of the contract that are about bits: any cut of the stream, either input
format, complex against two real handles, streams, reset, run-to-run and refusals.  `-m gpu`.

The bars are multiples of the yardstick, not the project's flat 1e-5: the float32 error of a recursion belongs to the
filter.  e32 and worst32 are the rel-RMS and the worst-sample error (both over the output's RMS) of the float32
sample-by-sample recursion (synth.iir_reference(..., np.float32)) against float64 on the same input, computed here:
    grid:    rel-RMS <= max(1e-6, 4 e32),    worst sample <= max(4e-6, 4 worst32)
    offset:  the same with 12 in place of 4
4: a numpy emulation of the block decomposition (runs of 16 and 64 from zero state, a sequential float32 fold, a float32
correction table) gave 0.5 to 1.3 times the yardstick's error on these filters; the factor leaves room for one more level.
12: with a constant offset the DC section's state holds the offset and the block correction is rounded at its scale; the
emulation gave up to 7.5 times the yardstick (the S = 5 cascade), 12 is that with 1.5x headroom.  tests/test_iir_host.py
caps the yardstick itself.  Every measured pair is printed beside its bar."""
import ctypes as C

import numpy as np
import pytest

from simplefe_amd import synth

pytestmark = pytest.mark.gpu
FILTERS = synth.iir_grid_filters()
CASCADE = "dc(0.999)+butter(8,0.1)"


@pytest.fixture(scope="module")
def api():
    from simplefe_amd import api as a
    return a


@pytest.fixture(scope="module")
def L():
    from simplefe_amd import lib
    return lib


@pytest.fixture(scope="module")
def G(api):
    return api.iir_plan(synth.iir_one_pole(0.5))[0]


def _streams(n, n_streams, first=0):
    return np.stack([synth.synth_cf32(n, ch=s, first_sample=first).view(np.complex64) for s in range(n_streams)])


def _errors(got, ref):
    """(rel-RMS, worst sample) of got against ref, both over ref's RMS."""
    err = np.abs(got.astype(ref.dtype) - ref)
    rms = np.sqrt(np.mean(np.abs(ref) ** 2))
    return np.sqrt(np.mean(err ** 2)) / rms, err.max() / rms


_refs = {}


def _yard(key, x, sos):
    """(float64 reference, float32 yardstick) of one input, computed once per key and left unchanged."""
    if key not in _refs:
        _refs[key] = (synth.iir_reference(x, sos), synth.iir_reference(x, sos, np.float32))
    return _refs[key]


def _check(tag, got, ref, y32, factor):
    rel, worst = _errors(got, ref)
    e32, w32 = _errors(y32, ref)
    bar_r, bar_w = max(1e-6, factor * e32), max(4e-6, factor * w32)
    print("iir %s: rel-RMS %.2e (yardstick %.2e, bar %.2e, %.2fx)  worst %.2e (yardstick %.2e, bar %.2e, %.2fx)"
          % (tag, rel, e32, bar_r, rel / e32, worst, w32, bar_w, worst / w32))
    assert rel <= bar_r and worst <= bar_w, (tag, rel, bar_r, worst, bar_w)


def _run_calls(api, f, x, cuts):
    """Feed (n_streams, n) x to handle f in calls of the given sizes (samples); returns the output, x's shape and dtype."""
    S, n = x.shape
    w = 2 if np.iscomplexobj(x) else 1
    d_in = api.DeviceArray.from_numpy(np.ascontiguousarray(x).view(np.float32))
    d_out = api.DeviceArray(S * n * w)
    pos = 0
    for c in cuts:
        assert f.process_stream(d_in.ptr + 4 * w * pos, c, d_out.ptr + 4 * w * pos, in_stride=n, out_stride=n) == c
        pos += c
    assert pos == n
    y = d_out.to_numpy().view(x.dtype).reshape(S, n).copy()
    d_in.free()
    d_out.free()
    return y


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("n_streams", [1, 3])
@pytest.mark.parametrize("name", list(FILTERS))
def test_parity_grid(api, G, name, n_streams):
    n = 3 * G
    x = _streams(n, 3)[:n_streams]
    ref, y32 = _yard(("grid", name), _streams(n, 3), FILTERS[name])
    f = api.Iir(FILTERS[name], n_streams=n_streams)
    d_in = api.DeviceArray.from_numpy(x.view(np.float32))
    sentinel = np.full(2 * (n_streams * n + 64), -77.0, np.float32)
    d_out = api.DeviceArray.from_numpy(sentinel)
    assert f.process_stream(d_in, n, d_out) == n
    y = d_out.to_numpy()
    assert np.array_equal(y[2 * n_streams * n:], sentinel[2 * n_streams * n:])      # the memory after the last sample is untouched
    y = y[:2 * n_streams * n].view(np.complex64).reshape(n_streams, n)
    for s in range(n_streams):
        _check("parity %s, %d stream(s), s=%d" % (name, n_streams, s), y[s], ref[s], y32[s], 4)
    f.close()
    d_in.free()
    d_out.free()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("name", ["dc(0.9999)", "dc(0.995)", CASCADE])
def test_a_constant_offset(api, L, G, name):
    n = 3 * G
    # as cf32: random bytes converted, plus a constant
    x = (synth.u8_to_cf32(synth.offset_bytes(n)) + np.complex64(0.3 + 0.2j))[None, :]
    assert abs(np.mean(x) - (0.3 + 0.2j)) < 0.03
    ref, y32 = _yard(("offset", name), x[0], FILTERS[name])
    _check("offset cf32 %s" % name, api.Iir(FILTERS[name]).filter(x[0]), ref, y32, 12)
    # as bytes biased to a mean near 166
    b = synth.offset_bytes(n, bias=38)
    assert abs(np.mean(b) - 166) < 1.5
    ref, y32 = _yard(("offset u8", name), synth.u8_to_cf32(b), FILTERS[name])
    f = api.Iir(FILTERS[name])
    f.set_input_format(L.FMT_U8)
    _check("offset u8 %s" % name, f.filter(b.reshape(n, 2)), ref, y32, 12)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("name", ["one_pole(0.999)", "dc(0.9999)"])
def test_an_impulse_across_blocks(api, G, name):
    sos = synth.iir_one_pole(0.999) if name.startswith("one") else FILTERS[name]
    (b0, b1, _, a1, _), = synth.iir_round(sos).astype(np.float64)
    n, at = 3 * G, G + 37
    x = np.zeros(n, np.complex64)
    x[at] = 1.0 - 0.5j
    y = api.Iir(sos).filter(x)
    assert not y[:at].any()                                 # exactly zero before the impulse
    # h[0] = b0, h[m] = (b1 - a1 b0) (-a1)^(m-1)
    m = np.arange(n - at)
    h = np.where(m == 0, b0, (b1 - a1 * b0) * (-a1) ** np.maximum(m - 1, 0))
    want = h * (1.0 - 0.5j)
    big = np.abs(h) > 1e-6 * np.abs(h).max()
    rel = np.abs(y[at:].astype(np.complex128) - want)[big] / np.abs(want)[big]
    print("iir impulse %s: %d of %d samples above 1e-6 of the peak, worst relative error %.2e (bar 1e-5)" % (name, big.sum(), big.size, rel.max()))
    assert big.sum() > 2 * G - 100 if name.startswith("dc") else big.sum() > G
    assert rel.max() <= 1e-5, (name, rel.max())


@pytest.mark.timeout(300)
@pytest.mark.parametrize("name", ["dc(0.9999)", CASCADE, "butter(16,0.1)"])
def test_cutting_the_stream_gives_the_same_bits(api, G, name):
    sos = FILTERS[name]
    x = _streams(12 * G, 2)
    one = _run_calls(api, api.Iir(sos, n_streams=2), x, [12 * G])
    ref, y32 = _yard(("cut", name), x[1], sos)
    _check("one call of 12 blocks, %s" % name, one[1], ref, y32, 4)
    for cuts in ([1] * 12, [3] * 4, [1, 4, 2, 5]):
        got = _run_calls(api, api.Iir(sos, n_streams=2), x, [c * G for c in cuts])
        assert np.array_equal(_bits(got), _bits(one)), (name, cuts)


@pytest.mark.timeout(300)
def test_cuts_across_the_groups_of_the_fold(api, G):
    """The fold over the blocks has two levels, grouped by absolute block index (128 blocks to a group): 300 blocks cut on
    group boundaries, beside them and far from them give the one-call bits, and so does block by block."""
    sos = FILTERS[CASCADE]
    nb = 300
    d = api.DeviceArray(2 * nb * G)
    d.fill_synth(synth.SEED, channel=3)
    x = d.to_numpy().view(np.complex64)[None, :]
    d.free()
    one = _run_calls(api, api.Iir(sos), x, [nb * G])
    for cuts in ([128, 128, 44], [64, 64, 172], [100, 28, 1, 127, 44], [127, 2, 171], [7] * 42 + [6], [1] * nb):
        assert sum(cuts) == nb
        got = _run_calls(api, api.Iir(sos), x, [c * G for c in cuts])
        assert np.array_equal(_bits(got), _bits(one)), cuts[:6]
    # the last window against the reference: the states have gone through two group boundaries
    at, lead = nb * G - 4096, 16384
    xw = x[0, at - lead:]
    ref = synth.iir_reference(xw, sos)[lead:]
    _check("300 blocks, last window", one[0, at:], ref, synth.iir_reference(xw, sos, np.float32)[lead:], 4)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("offset", [0, 2, 6])
@pytest.mark.parametrize("name", ["dc(0.995)", CASCADE])
def test_u8_input_equals_converted_cf32(api, L, G, name, offset):
    sos = FILTERS[name]
    n, cut = 3 * G, G
    b = synth.offset_bytes(n, seed=offset + 5)
    lib = L.load()
    # cf32 path: the library's own converter over an aligned copy of the bytes
    d_b = api.DeviceArray.from_bytes(b)
    d_f = api.DeviceArray(2 * n)
    assert lib.sfe_dsp_rx_u8_to_f32(d_b.ptr, d_f.ptr, 2 * n, None) == 0
    assert np.array_equal(_bits(d_f.to_numpy()), _bits(synth.u8_to_cf32(b)))
    d_ref = api.DeviceArray(2 * n)
    assert api.Iir(sos).process_stream(d_f, n, d_ref) == n
    want = d_ref.to_numpy()
    assert np.isfinite(want).all() and want.any()
    # u8 path: the same bytes at `offset` bytes past a 16-byte boundary, fed in two calls
    d_u = api.DeviceArray((2 * n + offset) // 4 + 8)
    assert d_u.ptr % 16 == 0
    assert lib.sfe_dsp_memcpy_h2d(d_u.ptr + offset, b.ctypes.data, 2 * n, None) == 0
    f = api.Iir(sos)
    f.set_input_format(L.FMT_U8)
    d_out = api.DeviceArray(2 * n)
    f.process_stream(d_u.ptr + offset, cut, d_out.ptr)
    f.process_stream(d_u.ptr + offset + 2 * cut, n - cut, d_out.ptr + 8 * cut)
    assert np.array_equal(_bits(d_out.to_numpy()), _bits(want)), (name, offset)
    # the format may change between two calls of one stream: cf32 first, then the bytes
    mix = api.Iir(sos)
    d_out.zero()
    mix.process_stream(d_f.ptr, cut, d_out.ptr)
    mix.set_input_format(L.FMT_U8)
    mix.process_stream(d_u.ptr + offset + 2 * cut, n - cut, d_out.ptr + 8 * cut)
    assert np.array_equal(_bits(d_out.to_numpy()), _bits(want)), (name, offset)
    # and filter() with (n, 2) bytes
    f2 = api.Iir(sos)
    f2.set_input_format(L.FMT_U8)
    assert np.array_equal(_bits(f2.filter(b.reshape(n, 2))), _bits(want))
    for d in (d_b, d_f, d_ref, d_u, d_out):
        d.free()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("name", ["dc(0.9999)", "butter(16,0.1)"])
def test_complex_equals_two_real_handles(api, G, name):
    sos = FILTERS[name]
    x = _streams(3 * G, 1)[0]
    y = api.Iir(sos).filter(x)
    re = api.Iir(sos, data_complex=False).filter(np.ascontiguousarray(x.real))
    im = api.Iir(sos, data_complex=False).filter(np.ascontiguousarray(x.imag))
    assert re.dtype == np.float32 and re.shape == x.shape
    assert np.array_equal(_bits(re), _bits(y.real)) and np.array_equal(_bits(im), _bits(y.imag))
    ref, y32 = _yard(("real", name), np.ascontiguousarray(x.real), sos)
    _check("real handle %s" % name, re, ref, y32, 4)


@pytest.mark.timeout(300)
def test_reset_and_streams_are_independent(api, G):
    sos = FILTERS[CASCADE]
    n = 3 * G
    x = _streams(n, 3)
    f = api.Iir(sos, n_streams=3)
    first = f.filter(_streams(n, 3, first=12345))           # something to forget
    f.reset()
    after_reset = f.filter(x)
    fresh = api.Iir(sos, n_streams=3).filter(x)
    assert fresh.shape == (3, n)
    assert np.array_equal(_bits(after_reset), _bits(fresh))
    assert not np.array_equal(_bits(first), _bits(fresh))
    # without the reset the state carries on: the second call of one handle is not a fresh handle's
    g = api.Iir(sos, n_streams=3)
    g.filter(x)
    assert not np.array_equal(_bits(g.filter(x)), _bits(fresh))
    for s in range(3):
        alone = api.Iir(sos).filter(x[s])
        assert np.array_equal(_bits(alone), _bits(fresh[s])), s
    ref, y32 = _yard(("streams", 1), x[1], sos)
    _check("stream 1 of 3", fresh[1], ref, y32, 4)


@pytest.mark.timeout(300)
def test_the_same_call_gives_the_same_bits_every_run(api, G):
    sos = FILTERS["butter(16,0.1)"]
    x = _streams(12 * G, 2)
    runs = [_run_calls(api, api.Iir(sos, n_streams=2), x, [12 * G]) for _ in range(3)]
    assert np.array_equal(_bits(runs[0]), _bits(runs[1])) and np.array_equal(_bits(runs[0]), _bits(runs[2]))


@pytest.mark.timeout(300)
def test_windows_of_a_large_call(api, G):
    """2^24 samples in one call: a fold over thousands of blocks and a grid larger than the chip.  Each window's reference
    starts from zero state 16 384 samples earlier: at pole radius <= 0.995 the forgotten past is below 1e-30."""
    sos = np.vstack([synth.iir_dc_blocker(0.995), synth.iir_butter_lowpass(8, 0.1)])
    poles = np.concatenate([np.roots([1.0, a1, a2]) for _, _, _, a1, a2 in synth.iir_round(sos).astype(np.float64)])
    assert np.abs(poles).max() <= 0.995 + 1e-6
    n, W, lead = 1 << 24, 4096, 16384
    d_in = api.DeviceArray(2 * n)
    d_in.fill_synth(synth.SEED)
    d_out = api.DeviceArray(2 * n)
    f = api.Iir(sos)
    assert f.process_stream(d_in, n, d_out) == n
    for at in (0, n // 2 - 1234, n - W):
        y = d_out.to_numpy(2 * W, offset=2 * at).view(np.complex64)
        first = max(0, at - lead)
        x = synth.synth_cf32(at + W - first, first_sample=first).view(np.complex64)
        ref = synth.iir_reference(x, sos)[at - first:]
        y32 = synth.iir_reference(x, sos, np.float32)[at - first:]
        _check("large call, window at %d" % at, y, ref, y32, 4)
    f.close()
    d_in.free()
    d_out.free()


@pytest.mark.timeout(300)
def test_refusals_launch_nothing(api, L, G):
    sos = FILTERS["butter(4,0.025)"]
    n = 3 * G
    x = _streams(n, 1)
    f = api.Iir(sos)
    d_in = api.DeviceArray.from_numpy(np.concatenate([x.view(np.float32).ravel(), np.zeros(64, np.float32)]))
    sentinel = np.full(2 * n + 64, 1234.5, np.float32)
    d_out = api.DeviceArray.from_numpy(sentinel)
    lib = L.load()
    k = C.c_size_t(7)

    def call(pi, n_in, in_stride, po, out_stride, stream=None, h=None):
        return lib.sfe_dsp_iir_process_stream(h or f._h, pi, n_in, in_stride, po, out_stride, C.byref(k), stream)

    assert call(d_in.ptr, n - 1, n, d_out.ptr, n) == L.SFE_EINVAL                 # n_in not a multiple of G
    assert call(d_in.ptr, n - G // 2, n, d_out.ptr, n) == L.SFE_EINVAL
    assert call(d_in.ptr + 4, n, n, d_out.ptr, n) == L.SFE_EINVAL                 # misaligned cf32 input
    assert call(d_in.ptr, n, n, d_out.ptr + 4, n) == L.SFE_EINVAL                 # misaligned output
    assert call(d_in.ptr, n, n, d_in.ptr + 8 * 16, n) == L.SFE_EINVAL             # output overlaps input
    assert call(d_in.ptr, n, n, d_out.ptr, n - 1) == L.SFE_ERANGE                 # out_stride one sample short
    assert call(None, n, n, d_out.ptr, n) == L.SFE_EINVAL                         # null input
    assert call(d_in.ptr, n, n, None, n) == L.SFE_EINVAL                          # null output
    assert k.value == 0
    assert lib.sfe_dsp_iir_set_input_format(f._h, 7) == L.SFE_EINVAL              # a bad format: the handle stays cf32
    assert lib.sfe_dsp_iir_set_input_format(f._h, L.FMT_TX10) == L.SFE_EINVAL
    real = api.Iir(sos, data_complex=False)
    assert lib.sfe_dsp_iir_set_input_format(real._h, L.FMT_U8) == L.SFE_EINVAL    # bytes are (I,Q) pairs
    assert call(d_in.ptr + 2, G, G, d_out.ptr, G, h=real._h) == L.SFE_EINVAL      # ... and float32 wants 4-byte alignment
    # a capturing stream: the sample counter lives on the host
    hip = C.CDLL("libamdhip64.so")
    for name, args in (("hipStreamCreate", [C.POINTER(C.c_void_p)]), ("hipStreamBeginCapture", [C.c_void_p, C.c_int]),
                       ("hipStreamEndCapture", [C.c_void_p, C.POINTER(C.c_void_p)]), ("hipGraphDestroy", [C.c_void_p]),
                       ("hipStreamDestroy", [C.c_void_p])):
        fn = getattr(hip, name)
        fn.argtypes, fn.restype = args, C.c_int
    s = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(s)) == 0
    assert hip.hipStreamBeginCapture(s, 2) == 0            # relaxed mode: the refused call launches nothing
    try:
        rc = call(d_in.ptr, n, n, d_out.ptr, n, s.value)
    finally:
        g = C.c_void_p()
        hip.hipStreamEndCapture(s, C.byref(g))
    if g.value:
        hip.hipGraphDestroy(g)
    hip.hipStreamDestroy(s)
    assert rc == L.SFE_ESTATE and k.value == 0
    api.sync()
    assert np.array_equal(d_out.to_numpy(), sentinel)
    assert np.array_equal(d_in.to_numpy(2 * n), x.view(np.float32).ravel())
    # nothing advanced either: the next good call is a fresh handle's, and matches the reference of the uncut stream
    assert f.process_stream(d_in, n, d_out) == n
    got = d_out.to_numpy(2 * n).view(np.complex64)
    assert np.array_equal(_bits(got), _bits(api.Iir(sos).filter(x[0])))
    ref, y32 = _yard(("refusals", 0), x[0], sos)
    _check("after the refusals", got, ref, y32, 4)
