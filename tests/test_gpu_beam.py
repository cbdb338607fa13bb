"""The multi-stream beamformer / stream-mixing bank on the GPU (sfe_dsp_beam_*, csrc/beam.hip) against the float64
reference of its law (synth.beam_reference), and the parts of the contract that are about bits: any cut of the stream,
any element-aligned address and stride, either input format, bands against one-band handles, exact selections,
set_weights against a fresh handle, and run-to-run determinism.

The accuracy bar is derived, not measured.  An output float is a float32 dot product of n = 2S terms on the rounded
matrix R; in any order, fused or not, it errs by at most gamma_n sum|R||x| with gamma_n ~ n 2^-24.  The reference is
rounded to float32 for the comparison, which costs it one more rounding of the result (covered by the factor 2):

    |y - ref| <= 2 (2S + 1) 2^-24 sum_k |R[i][k]| |x[k]| + 1e-30        per output float

beside the project's usual rel-RMS <= 1e-5.  The input is the synthetic stream (multiples of 2^-23 in [-1, 1): bounded,
no denormals) or uniformly random (I,Q) bytes."""
import ctypes as C

import numpy as np
import pytest

from simplefe_amd import synth

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1), (2, 3), (3, 2), (5, 5), (8, 8), (16, 4), (17, 17), (33, 9), (64, 64)]     # (S, B)
SIZES = [1, 63, 64, 65, 1000, 4097]
NMAX = max(SIZES)
MARGIN = 4096                   # guard bytes on both sides of every row
SENT = np.float32(-7654.25)


@pytest.fixture(scope="module")
def api():
    from simplefe_amd import api as a
    return a


@pytest.fixture(scope="module")
def L():
    from simplefe_amd import lib
    return lib


@pytest.fixture(scope="module")
def hip():
    h = C.CDLL("libamdhip64.so")
    for name, args in (("hipStreamCreate", [C.POINTER(C.c_void_p)]), ("hipStreamBeginCapture", [C.c_void_p, C.c_int]),
                       ("hipStreamEndCapture", [C.c_void_p, C.POINTER(C.c_void_p)]), ("hipGraphDestroy", [C.c_void_p]),
                       ("hipStreamDestroy", [C.c_void_p]), ("hipGetDevice", [C.POINTER(C.c_int)]), ("hipSetDevice", [C.c_int]),
                       ("hipGraphGetNodes", [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)])):
        fn = getattr(h, name)
        fn.argtypes, fn.restype = args, C.c_int
    return h


def _weights(S, B, M, seed):
    """(M, B, S) complex64, every entry non-zero, rows of about unit gain."""
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal((M, B, S)) + 1j * rng.standard_normal((M, B, S))) / np.sqrt(2 * S)).astype(np.complex64)


_inputs = {}


def _input(S, M, n, u8):
    """(what is uploaded, the same as complex64), (S, M, n): the synthetic stream, or random bytes and their conversion.
    Computed once per key and left unchanged."""
    key = (S, M, n, u8)
    if key not in _inputs:
        if u8:
            b = synth.offset_bytes(S * M * n, seed=synth.SEED + 7 * S + M).reshape(S, M, 2 * n)
            _inputs[key] = (b, synth.u8_to_cf32(b.reshape(-1)).reshape(S, M, n))
        else:
            x = np.stack([synth.synth_cf32(M * n, ch=s).view(np.complex64).reshape(M, n) for s in range(S)])
            _inputs[key] = (x, x)
    return _inputs[key]


def _bits(y):
    return np.ascontiguousarray(y).view(np.uint32)


def _bound(R, x):
    """The per-float bound of the module's docstring for x (S, M, n): (B, M, n, 2) float64."""
    M, B2, S2 = R.shape
    X = np.empty((M, S2, x.shape[2]))
    X[:, 0::2] = np.abs(x.real).transpose(1, 0, 2)
    X[:, 1::2] = np.abs(x.imag).transpose(1, 0, 2)
    A = np.matmul(np.abs(R).astype(np.float64), X)                  # (M, 2B, n)
    A = np.stack([A[:, 0::2], A[:, 1::2]], axis=-1).transpose(1, 0, 2, 3)
    return 2.0 * (S2 + 1) * 2.0 ** -24 * A + 1e-30


def _check(tag, got, ref, bound):
    """got (B, M, n) complex64 against ref complex128, rounded to float32 for the comparison."""
    g = np.ascontiguousarray(got).view(np.float32).reshape(got.shape + (2,)).astype(np.float64)
    r32 = ref.astype(np.complex64)
    r = np.ascontiguousarray(r32).view(np.float32).reshape(ref.shape + (2,)).astype(np.float64)
    err = np.abs(g - r)
    worst = float((err / bound).max())
    rel = synth.rel_rms(g, r)
    print("beam %s: worst error %.3f of its bound, rel-RMS %.2e (bar 1e-5)" % (tag, worst, rel))
    assert np.isfinite(g).all(), tag
    assert (err <= bound).all(), (tag, worst)
    assert rel <= 1e-5, (tag, rel)


class Rows:
    """A device buffer of `rows` rows of n elements of `esz` bytes, the first `shift` elements behind a guard, with at
    least MARGIN guard bytes in front of every row and behind the last (the stride is n + extra + the guard); guards and
    gaps hold the repeated `fill_bytes` pattern."""

    def __init__(self, api, rows, n, esz, fill_bytes, extra=0, shift=0):
        self.api, self.rows, self.n, self.esz = api, rows, n, esz
        self.stride = n + extra + -(-MARGIN // esz)                 # elements: a row's payload, slack, then a guard
        self.off = MARGIN + shift * esz                             # bytes: the first row starts behind a guard
        self.nbytes = -(-(self.off + rows * self.stride * esz + MARGIN) // 4) * 4
        self.host = np.frombuffer(np.resize(np.frombuffer(fill_bytes, np.uint8), self.nbytes).tobytes(), np.uint8).copy()
        self.d = api.DeviceArray(self.nbytes // 4)
        self.ptr = self.d.ptr + self.off

    def payload(self):
        """A (rows, n * esz) uint8 view of the host image's payload."""
        v = self.host[self.off:self.off + self.rows * self.stride * self.esz].reshape(self.rows, self.stride * self.esz)
        return v[:, :self.n * self.esz]

    def upload(self, a):
        self.payload()[:] = np.ascontiguousarray(a).view(np.uint8).reshape(self.rows, self.n * self.esz)
        self.api.check(self.d._L.sfe_dsp_memcpy_h2d(self.d.ptr, self.host.ctypes.data, self.nbytes, None))
        self.api.sync()
        return self

    def download(self):
        """(payload as (rows, n * esz) bytes, True when every byte outside the payload is what was uploaded)."""
        got = np.empty(self.nbytes, np.uint8)
        self.api.check(self.d._L.sfe_dsp_memcpy_d2h(got.ctypes.data, self.d.ptr, self.nbytes, None))
        self.api.sync()
        want = self.host.copy()
        lo, hi = self.off, self.off + self.rows * self.stride * self.esz
        body = got[lo:hi].reshape(self.rows, -1)
        wbody = want[lo:hi].reshape(self.rows, -1)
        pay = body[:, :self.n * self.esz].copy()
        intact = (np.array_equal(got[:lo], want[:lo]) and np.array_equal(got[hi:], want[hi:])
                  and np.array_equal(body[:, self.n * self.esz:], wbody[:, self.n * self.esz:]))
        return pay, intact

    def free(self):
        self.d.free()


NAN_BYTES = np.array([0x7fc00001, 0xffc12345, 0x7f800001, 0xffffffff], np.uint32).tobytes()      # quiet, signalling, all ones
FF_BYTES = b"\xff"
SENT_BYTES = np.array([SENT], np.float32).tobytes()


def _guarded(api, beam, up, n, u8, extra_in=0, extra_out=0, shift_in=0, shift_out=0):
    """One call over guarded buffers: (output (B, M, n) complex64, guards intact)."""
    S, B, M = beam.n_in, beam.n_beams, beam.n_bands
    src = Rows(api, S * M, n, 2 if u8 else 8, FF_BYTES if u8 else NAN_BYTES, extra_in, shift_in).upload(up)
    dst = Rows(api, B * M, n, 8, SENT_BYTES, extra_out, shift_out).upload(np.full((B * M, 2 * n), SENT, np.float32))
    try:
        assert beam.process_stream(src.ptr, n, dst.ptr, in_stride=src.stride, out_stride=dst.stride) == n
        api.sync()
        pay, intact = dst.download()
        _, in_intact = src.download()
    finally:
        src.free()
        dst.free()
    return pay.view(np.complex64).reshape(B, M, n), intact and in_intact


@pytest.mark.parametrize("M", [1, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_accuracy_against_float64(api, L, shape, M):
    S, B = shape
    W, V = _weights(S, B, M, 100 * S + B), _weights(S, B, M, 7 + 100 * S + B)
    for v in (None, V):
        beam = api.Beam(W, v)
        R = api.beam_plan(W, v)
        for u8 in (False, True):
            beam.set_input_format(L.FMT_U8 if u8 else L.FMT_F32)
            up, x = _input(S, M, NMAX, u8)
            ref, bound = synth.beam_reference(x, W, v), _bound(R, x)
            d_in = api.DeviceArray.from_bytes(up) if u8 else api.DeviceArray.from_numpy(up.view(np.float32))
            d_out = api.DeviceArray(B * M * NMAX * 2)
            for n in SIZES:                                         # a prefix of every row: the strides stay NMAX
                assert beam.process_stream(d_in, n, d_out, in_stride=NMAX, out_stride=NMAX) == n
                got = d_out.to_numpy().view(np.complex64).reshape(B, M, NMAX)[:, :, :n]
                _check("S=%d B=%d M=%d n=%d %s %s" % (S, B, M, n, "u8" if u8 else "cf32", "W" if v is None else "W+V"), got,
                       ref[:, :, :n], bound[:, :, :n])
            d_in.free()
            d_out.free()
        beam.close()


def test_selection_is_exact(api):
    """Contract 4, and the layout test: a transposed tile or a swapped re / im lane cannot pass it."""
    S, B, n = 5, 7, 1000
    pick = [4, 0, 2, 2, 1, 3, 0]
    sel = np.zeros((B, S), np.complex64)
    sel[np.arange(B), pick] = 1.0
    _, x = _input(S, 1, NMAX, False)
    x = np.ascontiguousarray(x[:, 0, :n])
    # finite and without a zero: a sum cannot return the sign of a zero (0 + -0 is +0), so -0 is outside the contract
    assert np.isfinite(x.view(np.float32)).all() and (x.view(np.float32) != 0).all()
    assert len({x[s].tobytes() for s in range(S)}) == S             # the streams differ
    direct = api.Beam(sel).mix(x)
    assert np.array_equal(_bits(direct), _bits(x[pick]))
    conj = api.Beam(np.zeros_like(sel), sel).mix(x)
    assert np.array_equal(_bits(conj), _bits(np.conj(x[pick])))
    assert not np.array_equal(_bits(conj), _bits(direct))


@pytest.mark.parametrize("u8", [False, True], ids=["cf32", "u8"])
@pytest.mark.parametrize("n", [1, 65, 1000])
@pytest.mark.parametrize("shape", [(3, 2), (17, 17)], ids=str)
def test_guards(api, L, shape, n, u8):
    """NaN bit patterns (bytes 0xFF for u8: they convert to 1.0, not to the zero a padding lane must see) all around every
    input row, a sentinel all around every output row and in the gaps of out_stride > n_in: every output is finite and
    within its bound, every sentinel intact."""
    S, B = shape
    M = 2
    W, V = _weights(S, B, M, 1000 + S), _weights(S, B, M, 2000 + S)
    beam = api.Beam(W, V)
    beam.set_input_format(L.FMT_U8 if u8 else L.FMT_F32)
    up, x = _input(S, M, NMAX, u8)
    up, x = np.ascontiguousarray(up[:, :, :(2 if u8 else 1) * n]), np.ascontiguousarray(x[:, :, :n])
    if u8:
        assert np.array_equal(synth.u8_to_cf32(up.reshape(-1)).reshape(S, M, n), x)
    got, intact = _guarded(api, beam, up, n, u8, extra_in=3, extra_out=5)
    assert intact
    _check("guards S=%d B=%d n=%d %s" % (S, B, n, "u8" if u8 else "cf32"), got, synth.beam_reference(x, W, V),
           _bound(api.beam_plan(W, V), x))


CUTS = [1, 2, 63, 64, 65, 129, 4095]


@pytest.mark.parametrize("u8", [False, True], ids=["cf32", "u8"])
@pytest.mark.parametrize("shape", [(17, 17, 1), (8, 8, 4)], ids=str)
def test_any_cut_address_and_stride_gives_the_same_bits(api, L, shape, u8):
    S, B, M = shape
    n = 10000
    W, V = _weights(S, B, M, 31), _weights(S, B, M, 32)
    beam = api.Beam(W, V)
    beam.set_input_format(L.FMT_U8 if u8 else L.FMT_F32)
    up, x = _input(S, M, n, u8)
    one = beam.mix(up)
    _check("one call S=%d B=%d M=%d %s" % (S, B, M, "u8" if u8 else "cf32"), one, synth.beam_reference(x, W, V),
           _bound(api.beam_plan(W, V), x))
    # cut at [1, 2, 63, 64, 65, 129, 4095, rest]: every call reads and writes its piece of the same two buffers
    esz, w = (2, 1) if u8 else (8, 2)
    d_in = api.DeviceArray.from_bytes(up) if u8 else api.DeviceArray.from_numpy(up.view(np.float32))
    d_out = api.DeviceArray(B * M * n * 2)
    at = 0
    for m in CUTS + [n - sum(CUTS)]:
        assert beam.process_stream(d_in.ptr + at * esz, m, d_out.ptr + at * 8, in_stride=n, out_stride=n) == m
        at += m
    assert at == n
    cut = d_out.to_numpy().view(np.complex64).reshape(B, M, n)
    assert np.array_equal(_bits(cut), _bits(one))
    d_in.free()
    d_out.free()
    # the same data 1, 2 and 3 samples into larger buffers with other strides (u8: an odd 2-byte offset at shift 1 and 3)
    for shift in (1, 2, 3):
        got, intact = _guarded(api, beam, up, n, u8, extra_in=shift + 2, extra_out=7 - shift, shift_in=shift, shift_out=4 - shift)
        assert intact and np.array_equal(_bits(got), _bits(one)), shift
    beam.close()


def test_u8_gives_the_bits_of_cf32_on_the_converted_samples(api, L):
    """Contract 2, with the format changing between two calls of one handle."""
    S, B, M, n = 17, 9, 2, 1000
    W, V = _weights(S, B, M, 41), _weights(S, B, M, 42)
    up, x = _input(S, M, n, True)
    beam = api.Beam(W, V)
    first = beam.mix(x)
    beam.set_input_format(L.FMT_U8)
    second = beam.mix(up)
    beam.set_input_format(L.FMT_F32)
    third = beam.mix(x)
    assert np.array_equal(_bits(second), _bits(first)) and np.array_equal(_bits(third), _bits(first))
    assert np.abs(first).max() > 0


def test_a_band_is_a_one_band_handle(api):
    """Contract 3; and the bands' outputs differ, so the band index is not ignored."""
    S, B, M, n = 17, 17, 4, 1000
    W, V = _weights(S, B, M, 51), _weights(S, B, M, 52)
    _, x = _input(S, M, n, False)
    all_bands = api.Beam(W, V).mix(x)
    same_input = np.ascontiguousarray(np.broadcast_to(x[:, :1], x.shape))
    mixed = api.Beam(W, V).mix(same_input)
    for k in range(M):
        alone = api.Beam(W[k], V[k]).mix(np.ascontiguousarray(x[:, k]))
        assert np.array_equal(_bits(all_bands[:, k]), _bits(alone)), k
        for k2 in range(k):
            assert not np.array_equal(mixed[:, k], mixed[:, k2]), (k, k2)        # one input, different weights


def test_set_weights_is_a_fresh_handle(api):
    S, B, M, n = 8, 8, 4, 4097
    W0, V0, W1, V1 = (_weights(S, B, M, 60 + i) for i in range(4))
    _, x = _input(S, M, n, False)
    beam = api.Beam(W0, V0)
    d_in = api.DeviceArray.from_numpy(x.view(np.float32))
    d_a, d_b = api.DeviceArray(B * M * n * 2), api.DeviceArray(B * M * n * 2)
    assert beam.process_stream(d_in, n, d_a) == n
    beam.set_weights(W1, V1)                            # enqueued behind nothing it could change: the first call is done
    assert beam.process_stream(d_in, n, d_b) == n
    first, second = d_a.to_numpy().view(np.uint32), d_b.to_numpy().view(np.uint32)
    assert np.array_equal(second, _bits(api.Beam(W1, V1).mix(x)).ravel())
    assert np.array_equal(first, _bits(api.Beam(W0, V0).mix(x)).ravel())
    assert not np.array_equal(first, second)
    beam.set_weights(W0)                                # V absent again: all zero
    assert np.array_equal(_bits(beam.mix(x)), _bits(api.Beam(W0).mix(x)))
    with pytest.raises(api.SfeError):
        bad = W0.copy()
        bad[1, 2, 3] = np.nan
        beam.set_weights(bad)
    assert np.array_equal(_bits(beam.mix(x)), _bits(api.Beam(W0).mix(x)))       # a refused retune changes nothing
    for d in (d_in, d_a, d_b):
        d.free()


def test_the_same_call_gives_the_same_bits(api):
    S, B, M, n = 33, 9, 2, 4097
    W, V = _weights(S, B, M, 71), _weights(S, B, M, 72)
    _, x = _input(S, M, n, False)
    beam = api.Beam(W, V)
    runs = [_bits(beam.mix(x)) for _ in range(3)]
    assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], runs[2])


def test_chan_beam_combine_share_their_layouts(api):
    """chan -> beam -> combine over device buffers with no copy between them: chan's output rows (s M + k) are beam's
    input rows, beam's output rows (b M + k) are combine's input rows.  Four whole-sample delays of one signal are
    undone per band and summed.  About the three layouts fitting; nothing here asserts beam-pattern physics."""
    M, D, S = 16, 8, 4
    h, g = synth.lowpass_taps(16 * M + 1, 2.0 / M), synth.lowpass_taps(16 * M + 1, 1.0 / M)
    delays = [0, 3, 5, 10]
    n = 4096
    base = synth.synth_cf32(n, ch=9).view(np.complex64)
    x = np.zeros((S, n), np.complex64)
    for s, d in enumerate(delays):
        x[s, d:] = base[:n - d]
    k = np.arange(M)
    W = np.stack([np.exp(2j * np.pi * k * d / M) / S for d in delays], axis=1)[:, None, :].astype(np.complex64)    # (M, 1, S)
    no = n // D
    chan, beam, comb = api.Chan(h, M, D, n_streams=S), api.Beam(W), api.Combiner(g, M, D)
    d_x = api.DeviceArray.from_numpy(x.view(np.float32))
    d_c, d_b, d_y = api.DeviceArray(S * M * no * 2), api.DeviceArray(M * no * 2), api.DeviceArray(n * 2)
    assert chan.process_stream(d_x, n, d_c, out_stride=no) == no
    assert beam.process_stream(d_c, no, d_b, in_stride=no, out_stride=no) == no
    assert comb.process_stream(d_b, no, d_y, in_stride=no) == n
    got = d_y.to_numpy().view(np.complex64)
    X = np.stack([synth.chan_reference(x[s], h, M, D) for s in range(S)])              # (S, M, no)
    Y = synth.beam_reference(X, W)                                                      # (1, M, no)
    ref = synth.combine_reference(Y[0], g, M, D)
    rel = synth.rel_rms(got.view(np.float32), ref.astype(np.complex64).view(np.float32))
    print("chan -> beam -> combine: rel-RMS %.2e (bar 1e-5)" % rel)
    assert np.abs(ref).max() > 1e-3 and rel <= 1e-5
    for d in (d_x, d_c, d_b, d_y):
        d.free()


def test_refusals_launch_nothing(api, L, hip):
    S, B, M, n = 3, 2, 2, 256
    W = _weights(S, B, M, 81)
    up8, _ = _input(S, M, n, True)
    _, x = _input(S, M, n, False)
    beam = api.Beam(W)
    d_in = api.DeviceArray.from_numpy(np.concatenate([x.view(np.float32).ravel(), np.zeros(64, np.float32)]))
    sentinel = np.full(B * M * n * 2 + 64, SENT, np.float32)
    d_out = api.DeviceArray.from_numpy(sentinel)
    lib = L.load()
    k = C.c_size_t(7)

    def call(pi, n_in, in_stride, po, out_stride, stream=None, h=None):
        return lib.sfe_dsp_beam_process_stream(h or beam._h, pi, n_in, in_stride, po, out_stride, C.byref(k), stream)

    assert call(d_in.ptr, n, n, d_out.ptr, n - 1) == L.SFE_ERANGE                   # out_stride one sample short
    assert call(d_in.ptr, n, n, d_in.ptr + 8 * 16, n) == L.SFE_EINVAL               # output overlaps input
    assert call(d_in.ptr + 4, n, n, d_out.ptr, n) == L.SFE_EINVAL                   # misaligned cf32 input
    assert call(d_in.ptr, n, n, d_out.ptr + 4, n) == L.SFE_EINVAL                   # misaligned output
    assert call(d_in.ptr, n, n - 1, d_out.ptr, n) == L.SFE_EINVAL                   # in_stride one sample short
    assert call(None, n, n, d_out.ptr, n) == L.SFE_EINVAL                           # null input
    assert call(d_in.ptr, n, n, None, n) == L.SFE_EINVAL                            # null output
    assert call(d_in.ptr, 1 << 31, 1 << 31, d_out.ptr, 1 << 31) == L.SFE_EINVAL     # 2^31 samples
    assert lib.sfe_dsp_beam_process_stream(beam._h, d_in.ptr, n, n, d_out.ptr, n, None, None) == L.SFE_EINVAL       # no counter
    beam.set_input_format(L.FMT_U8)
    assert call(d_in.ptr + 1, n, n, d_out.ptr, n) == L.SFE_EINVAL                   # an odd u8 address
    beam.set_input_format(L.FMT_F32)
    assert lib.sfe_dsp_beam_set_input_format(beam._h, 7) == L.SFE_EINVAL            # a bad format: the handle stays cf32
    assert lib.sfe_dsp_beam_set_input_format(beam._h, L.FMT_TX10) == L.SFE_EINVAL
    assert k.value == 0
    assert call(d_in.ptr, 0, 0, d_out.ptr, 0) == L.SFE_OK and k.value == 0          # n_in = 0: a no-op
    # a capturing stream: refused, and the capture ends as an empty graph
    s = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(s)) == 0
    assert hip.hipStreamBeginCapture(s, 2) == 0            # relaxed mode: the refused call launches nothing
    try:
        rc = call(d_in.ptr, n, n, d_out.ptr, n, s.value)
        msg = lib.sfe_dsp_last_error()
    finally:
        g = C.c_void_p()
        ended = hip.hipStreamEndCapture(s, C.byref(g))
    nodes = C.c_size_t(0)
    if g.value:
        assert hip.hipGraphGetNodes(g, None, C.byref(nodes)) == 0
        hip.hipGraphDestroy(g)
    hip.hipStreamDestroy(s)
    assert rc == L.SFE_ESTATE and k.value == 0 and b"graph capture is not supported" in msg
    assert ended == 0 and (not g.value or nodes.value == 0)
    # a live handle of another block is refused by every beam function, and beam's destroy frees nothing of it
    other = api.Iir(synth.iir_dc_blocker(0.995))
    wp = W.view(np.float32).ctypes.data_as(C.POINTER(C.c_float))
    assert call(d_in.ptr, n, n, d_out.ptr, n, h=other._h) == L.SFE_EINVAL and k.value == 0
    assert lib.sfe_dsp_beam_set_input_format(other._h, L.FMT_F32) == L.SFE_EINVAL
    assert lib.sfe_dsp_beam_set_weights(other._h, wp, None) == L.SFE_EINVAL
    assert lib.sfe_dsp_beam_destroy(other._h) == L.SFE_OK
    blk = other.block
    assert np.isfinite(other.filter(x[0, 0, :blk])).all()                          # still alive
    assert lib.sfe_dsp_iir_process_stream(beam._h, d_in.ptr, blk, blk, d_out.ptr, blk, C.byref(k), None) == L.SFE_EINVAL
    api.sync()
    assert np.array_equal(d_out.to_numpy(), sentinel)
    assert np.array_equal(d_in.to_numpy(x.size * 2), x.view(np.float32).ravel())
    # the next good call is a fresh handle's
    assert beam.process_stream(d_in, n, d_out) == n
    got = d_out.to_numpy(B * M * n * 2).view(np.complex64).reshape(B, M, n)
    assert np.array_equal(_bits(got), _bits(api.Beam(W).mix(x)))
    assert np.array_equal(d_out.to_numpy()[B * M * n * 2:], sentinel[B * M * n * 2:])
    d_in.free()
    d_out.free()


def test_create_leaves_the_current_device(api, hip):
    def current():
        d = C.c_int(-1)
        assert hip.hipGetDevice(C.byref(d)) == 0
        return d.value

    n_dev = api.device_count()
    assert hip.hipSetDevice(0) == 0
    W = synth.beam_steering_weights(4, 2)
    for device in range(min(n_dev, 2)):
        beam = api.Beam(W, device=device)
        assert current() == 0, device
        beam.set_weights(W)
        assert current() == 0, device
        beam.close()
        assert current() == 0, device
    with pytest.raises(api.SfeError):
        api.Beam(W, device=n_dev)                       # out of range: refused before anything is allocated
    with pytest.raises(api.SfeError):
        api.Beam(np.full((2, 4), np.inf, np.complex64))
    assert current() == 0
