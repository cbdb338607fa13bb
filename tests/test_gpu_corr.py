"""The streaming preamble correlator bank on the GPU (sfe_dsp_corr_*, csrc/corr.hip) against the float64 reference of its
contract (synth.corr_reference), and the parts of the contract that are about bits: peaks against the dense values, any
cut of the stream, either input format, streams and templates on their own, the gate, reset and refusals.  `-m gpu`.

TOL is the project's parity bar for every bank; here it is an absolute error on m, which is bounded by 1.  A float32
emulation of this law in numpy (overlap-save through 4096-point complex64 transforms, direct window energy) stayed
within 3.4e-7 of float64 for L = 13 ... 2049, so the bar has about 30x over float32 itself.  The GPU's worst case over
the parity grid is 3.2e-7 (L = 13; 2.4e-7 at L = 1, 2.3e-7 at L = 257, 6.1e-8 at L = 2049).

Inputs: synth.synth_cf32 noise; templates are (+-1 +- j) symbols drawn from the same generator; every one of the 16
templates is planted once in every stream, added at amplitude 1.0 for L <= 64, 0.5 for L <= 257, 0.25 above, at starts
spread evenly over the stream.  Each parity case first asserts on the float64 reference that the planted peak exceeds
every other value of its block by more than 0.05.  At L = 1 the law itself makes that impossible -- one sample is always
a multiple of a one-sample template, so m = 1 wherever the gate is open -- and the planted-start check is for L > 1; the
other two checks hold for every block of every case."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

from simplefe_amd import synth

pytestmark = pytest.mark.gpu
TOL = 1e-5
GATE = 1e-6
KMAX = 16
# The noise stream: at L = 13 a window of plain noise reaches m = 0.65 about once in 300 000 windows, the planted peaks
# are 0.6 to 0.8, and the grid looks at some 1.6 million windows per block size -- on most seeds the precondition fails in a
# block or two.  This seed was picked on the float64 reference alone: the first on which it holds in every case.
NOISE_SEED = synth.SEED + 77
PAD = 5             # sentinel elements after every output row
SENT = -77.0


@pytest.fixture(scope="module")
def api():
    from simplefe_amd import api as a
    return a


@pytest.fixture(scope="module")
def L():
    from simplefe_amd import lib
    return lib


def _advance(Lt):
    return 4096 - 256 * -(-(Lt - 1) // 256)


@functools.lru_cache(maxsize=None)
def _templates(Lt, K=KMAX):
    t = np.stack([synth.synth_cf32(Lt, ch=100 + k).view(np.complex64) for k in range(K)])
    return (np.where(t.real >= 0, 1.0, -1.0) + 1j * np.where(t.imag >= 0, 1.0, -1.0)).astype(np.complex64)


def _amp(Lt):
    return 1.0 if Lt <= 64 else 0.5 if Lt <= 257 else 0.25


def _starts(Lt, n, s):
    return [min(n - Lt, (k * (n - Lt)) // KMAX + 37 * s + 11) for k in range(KMAX)]


@functools.lru_cache(maxsize=8)
def _case(Lt, n, s):
    """Stream s of n samples with the 16 templates planted, and its float64 reference at block size n (the per-block
    peaks are taken from m by the caller).  Shared by the cases that differ in K and in the number of streams."""
    x = synth.synth_cf32(n, seed=NOISE_SEED, ch=s).view(np.complex64).copy()
    t = _templates(Lt)
    for k, p in enumerate(_starts(Lt, n, s)):
        x[p:p + Lt] += np.float32(_amp(Lt)) * t[k]
    m, _, _ = synth.corr_reference(x, t, n, GATE)
    m.setflags(write=False)
    x.setflags(write=False)
    return x, m


def _run(api, cr, x, cuts, dense=True, u8=None):
    """Feed (S, n) complex64 x -- or with u8 the (S, 2n) bytes -- to handle cr in calls of the given sizes (samples).
    Every output row is followed by PAD sentinels, checked here.  Returns (peak_val (S, K, nb) float32, peak_idx uint32,
    m (S, K, n) float32 or None)."""
    S, K, B = cr.n_streams, cr.n_templates, cr.block
    if u8 is None:
        n = x.shape[1]
        d_in = api.DeviceArray.from_numpy(np.ascontiguousarray(x).view(np.float32))
        esz = 8
    else:
        n = u8.shape[1] // 2
        d_in = api.DeviceArray.from_bytes(u8)
        esz = 2
    nb = n // B
    d_val = api.DeviceArray.from_numpy(np.full(S * K * (nb + PAD), SENT, np.float32))
    d_idx = api.DeviceArray.from_numpy(np.full(S * K * (nb + PAD), SENT, np.float32))
    d_m = api.DeviceArray.from_numpy(np.full(S * K * (n + PAD), SENT, np.float32)) if dense else None
    pos = 0
    for c in cuts:
        got = cr.process_stream(d_in.ptr + esz * pos, c, d_val.ptr + 4 * (pos // B), d_idx.ptr + 4 * (pos // B),
                                d_m.ptr + 4 * pos if dense else None, in_stride=n, peak_stride=nb + PAD, metric_stride=n + PAD)
        assert got == c // B
        pos += c
    assert pos == n
    val = d_val.to_numpy().reshape(S * K, nb + PAD)
    idx = d_idx.to_numpy().reshape(S * K, nb + PAD)
    assert np.all(val[:, nb:] == SENT) and np.all(idx[:, nb:] == SENT)
    m = None
    if dense:
        m = d_m.to_numpy().reshape(S * K, n + PAD)
        assert np.all(m[:, n:] == SENT)
        m = m[:, :n].reshape(S, K, n).copy()
        d_m.free()
    d_in.free()
    d_val.free()
    d_idx.free()
    return val[:, :nb].reshape(S, K, nb).copy(), idx[:, :nb].view(np.uint32).reshape(S, K, nb).copy(), m


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check_parity(Lt, K, B, x, val, idx, m, tag):
    """The three checks of a parity case on every stream, template and block; returns the worst dense and peak errors."""
    S, n = x.shape
    nb = n // B
    worst_m = worst_p = 0.0
    for s in range(S):
        xs, ref = _case(Lt, n, s)
        assert np.array_equal(xs, x[s])
        starts = _starts(Lt, n, s)
        for k in range(K):
            err = np.abs(m[s, k].astype(np.float64) - ref[k]).max()
            worst_m = max(worst_m, err)
            assert err <= TOL, (tag, s, k, err)
            blocks = ref[k].reshape(nb, B)
            for j in range(nb):
                top = blocks[j].max()
                perr = abs(float(val[s, k, j]) - top)
                worst_p = max(worst_p, perr)
                assert perr <= TOL, (tag, s, k, j, perr)
                assert idx[s, k, j] < B and blocks[j, idx[s, k, j]] >= top - 2 * TOL, (tag, s, k, j)
            if Lt > 1:
                end = starts[k] + Lt - 1
                j = end // B
                others = np.delete(blocks[j], end % B)
                assert blocks[j, end % B] > others.max() + 0.05, (tag, s, k, "precondition", blocks[j, end % B], others.max())
                assert j * B + int(idx[s, k, j]) - (Lt - 1) == starts[k], (tag, s, k)
    return worst_m, worst_p


GRID = [(Lt, ratio, S, K) for Lt, ratio in itertools.product((1, 13, 256, 257, 258, 2049), (1, 3)) for S in (1, 3) for K in (1, 3, 16)]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("Lt, ratio, S, K", GRID)
def test_parity_grid(api, Lt, ratio, S, K):
    B = ratio * _advance(Lt)
    n = 3 * B
    x = np.stack([_case(Lt, n, s)[0] for s in range(S)])
    cr = api.Corr(_templates(Lt)[:K], B, GATE, n_streams=S)
    val, idx, m = _run(api, cr, x, [n])
    cr.close()
    wm, wp = _check_parity(Lt, K, B, x, val, idx, m, (Lt, ratio, S, K))
    print("corr parity L=%d B=%dV S=%d K=%d: worst dense %.2e worst peak %.2e" % (Lt, ratio, S, K, wm, wp))


@pytest.mark.timeout(300)
@pytest.mark.parametrize("Lt", [16, 17])
def test_parity_on_both_sides_of_the_time_domain_threshold(api, Lt):
    B = _advance(Lt)
    n = 3 * B
    x = _case(Lt, n, 0)[0][None, :]
    cr = api.Corr(_templates(Lt)[:2], B, GATE)
    val, idx, m = _run(api, cr, x, [n])
    cr.close()
    wm, wp = _check_parity(Lt, 2, B, x, val, idx, m, (Lt,))
    print("corr parity L=%d: worst dense %.2e worst peak %.2e" % (Lt, wm, wp))


@pytest.mark.timeout(300)
@pytest.mark.parametrize("Lt, ratio", [(1, 1), (13, 3), (257, 1), (258, 3), (2049, 2)])
def test_peaks_are_the_maxima_of_the_dense_values(api, Lt, ratio):
    B = ratio * _advance(Lt)
    n = 3 * B
    S, K = 2, 3
    x = np.stack([_case(Lt, n, s)[0] for s in range(S)])
    val, idx, m = _run(api, api.Corr(_templates(Lt)[:K], B, GATE, n_streams=S), x, [n])
    blocks = m.reshape(S, K, 3, B)
    assert np.array_equal(_bits(val), _bits(blocks.max(axis=3)))
    assert np.array_equal(idx, blocks.argmax(axis=3).astype(np.uint32))
    val2, idx2, none = _run(api, api.Corr(_templates(Lt)[:K], B, GATE, n_streams=S), x, [n], dense=False)
    assert none is None
    assert np.array_equal(_bits(val2), _bits(val)) and np.array_equal(idx2, idx)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("ratio, second", [(1, 2000), (3, 2 * 3840 + 100)])
def test_the_first_of_two_equal_maxima_is_reported(api, ratio, second):
    """The template of length 13 twice in one block of an otherwise zero stream: in one slot, and two slots apart (the
    fold of the slot peaks breaks the tie)."""
    Lt, first = 13, 500
    B = ratio * _advance(Lt)
    t = _templates(Lt)[:1]
    x = np.zeros((1, 2 * B), np.complex64)
    for p in (first, second):
        x[0, B + p:B + p + Lt] = np.float32(0.5) * t[0]
    val, idx, m = _run(api, api.Corr(t, B, 1e-3), x, [2 * B])
    a, b = B + first + Lt - 1, B + second + Lt - 1
    assert _bits(m[0, 0, a:a + 1])[0] == _bits(m[0, 0, b:b + 1])[0]
    assert abs(float(m[0, 0, a]) - 1.0) <= TOL and m[0, 0].max() == m[0, 0, a]
    assert idx[0, 0, 1] == first + Lt - 1 and _bits(val[0, 0, 1:2])[0] == _bits(m[0, 0, a:a + 1])[0]
    assert val[0, 0, 0] == 0.0 and idx[0, 0, 0] == 0 and not m[0, 0, :B].any()      # a block of silence: the gate is shut
    ref, _, ri = synth.corr_reference(x[0], t, B, 1e-3)
    assert np.abs(m[0, 0] - ref[0]).max() <= TOL


@pytest.mark.timeout(300)
@pytest.mark.parametrize("Lt, ratio", [(257, 2), (2049, 1)])
def test_cutting_the_stream_gives_the_same_bits(api, Lt, ratio):
    B = ratio * _advance(Lt)
    n = 6 * B
    S, K = 2, 2
    x = np.stack([_case(Lt, n, s)[0] for s in range(S)])
    t = _templates(Lt)[:K]
    one = _run(api, api.Corr(t, B, GATE, n_streams=S), x, [n])
    for s in range(S):
        assert np.abs(one[2][s] - _case(Lt, n, s)[1][:K]).max() <= TOL
    for cuts in ([B, 2 * B, 3 * B], [B] * 6):
        got = _run(api, api.Corr(t, B, GATE, n_streams=S), x, cuts)
        for a, b in zip(got, one):
            assert np.array_equal(_bits(a), _bits(b)), (Lt, cuts)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("Lt, ratio", [(13, 1), (257, 2), (2049, 1)])
def test_u8_input_equals_converted_cf32(api, L, Lt, ratio):
    B = ratio * _advance(Lt)
    n = 4 * B
    S, K = 2, 2
    rng = np.random.default_rng(Lt)
    b = rng.integers(0, 256, size=(S, 2 * n), dtype=np.uint8)
    t = _templates(Lt)[:K]
    for s in range(S):      # the bytes of a planted template, so that there is something to find
        p = 1000 + s
        z = 0.25 * synth.synth_cf32(Lt, ch=7).view(np.complex64) + 0.5 * t[s]
        b[s, 2 * p:2 * (p + Lt)] = np.clip(np.round(z.view(np.float32) * 127.0 + 128.0), 0, 255).astype(np.uint8)
    lib = L.load()
    d_b = api.DeviceArray.from_bytes(b)
    d_f = api.DeviceArray(S * 2 * n)
    assert lib.sfe_dsp_rx_u8_to_f32(d_b.ptr, d_f.ptr, S * 2 * n, None) == 0
    xf = d_f.to_numpy().view(np.complex64).reshape(S, n)
    d_b.free()
    d_f.free()
    want = _run(api, api.Corr(t, B, GATE, n_streams=S), xf, [n])
    assert want[0].max() > 0.3 and np.isfinite(want[2]).all()
    cr = api.Corr(t, B, GATE, n_streams=S)
    cr.set_input_format(L.FMT_U8)
    got = _run(api, cr, None, [B, 3 * B], u8=b)
    for a, w in zip(got, want):
        assert np.array_equal(_bits(a), _bits(w)), Lt
    # the format may change between two calls of one stream: cf32 first, then the bytes
    mix = api.Corr(t, B, GATE, n_streams=S)
    first = _run(api, mix, xf[:, :2 * B], [2 * B])
    mix.set_input_format(L.FMT_U8)
    rest = _run(api, mix, None, [2 * B], u8=np.ascontiguousarray(b[:, 4 * B:]))
    for a, c, w in zip(first, rest, want):
        assert np.array_equal(_bits(np.concatenate([a, c], axis=2)), _bits(w)), Lt
    # and search() with (S, n, 2) bytes
    cr.reset()
    sv, si = cr.search(b.reshape(S, n, 2))
    assert np.array_equal(_bits(sv), _bits(want[0])) and np.array_equal(si, want[1])


@pytest.mark.timeout(300)
@pytest.mark.parametrize("Lt, ratio", [(13, 2), (257, 1), (2049, 2)])
def test_streams_and_templates_are_independent(api, Lt, ratio):
    B = ratio * _advance(Lt)
    n = 3 * B
    x = np.stack([_case(Lt, n, s)[0] for s in range(3)])
    t = _templates(Lt)[:3]
    full = _run(api, api.Corr(t, B, GATE, n_streams=3), x, [n])
    alone = _run(api, api.Corr(t, B, GATE), x[1:2], [n])
    for a, f in zip(alone, full):
        assert np.array_equal(_bits(a[0]), _bits(f[1])), Lt
    single = _run(api, api.Corr(t[2:3], B, GATE, n_streams=3), x, [n])
    for a, f in zip(single, full):
        assert np.array_equal(_bits(a[:, 0]), _bits(f[:, 2])), Lt


@pytest.mark.timeout(300)
def test_the_gate(api):
    Lt, gate = 64, 1e-3
    B = _advance(Lt)
    x = np.zeros((1, 4 * B), np.complex64)
    x[0, B:3 * B] = _case(Lt, 3 * B, 0)[0][:2 * B]
    t = _templates(Lt)[:2]
    xp = np.concatenate([np.zeros(Lt - 1), np.abs(x[0].astype(np.complex128)) ** 2])
    e = np.convolve(xp, np.ones(Lt), mode="valid")
    assert not np.any((e > gate / 2) & (e < 2 * gate))          # no window near the gate: float32 decides as float64 does
    shut = e <= gate
    assert shut[:B].all() and shut[3 * B + Lt:].all() and not shut[B + Lt:3 * B].any()
    ref, rv, ri = synth.corr_reference(x[0], t, B, gate)
    val, idx, m = _run(api, api.Corr(t, B, gate), x, [4 * B])
    for k in range(2):
        assert not m[0, k][shut].any() and not np.signbit(m[0, k][shut]).any()
        assert np.abs(m[0, k] - ref[k]).max() <= TOL
        assert val[0, k, 0] == 0.0 and idx[0, k, 0] == 0        # a block the gate shuts throughout
        assert np.abs(val[0, k] - rv[k]).max() <= TOL
        for j in (1, 2, 3):
            assert ref[k, j * B + idx[0, k, j]] >= rv[k, j] - 2 * TOL


@pytest.mark.timeout(300)
def test_reset_gives_a_fresh_handle(api):
    Lt = 258
    B = 2 * _advance(Lt)
    n = 2 * B
    x = np.stack([_case(Lt, n, s)[0] for s in range(2)])
    t = _templates(Lt)[:2]
    cr = api.Corr(t, B, GATE, n_streams=2)
    before = _run(api, cr, x[:, ::-1], [n])             # something to forget
    after_first = _run(api, cr, x, [n])                 # the history of the reversed stream leads this one
    cr.reset()
    after_reset = _run(api, cr, x, [n])
    fresh = _run(api, api.Corr(t, B, GATE, n_streams=2), x, [n])
    for a, f in zip(after_reset, fresh):
        assert np.array_equal(_bits(a), _bits(f))
    assert not np.array_equal(_bits(after_first[2]), _bits(fresh[2]))
    assert not np.array_equal(_bits(before[2]), _bits(fresh[2]))


@pytest.mark.timeout(300)
def test_refusals_launch_nothing(api, L):
    Lt = 257
    B = 2 * _advance(Lt)
    n = 2 * B
    K = 2
    x = _case(Lt, n, 0)[0]
    t = _templates(Lt)[:K]
    cr = api.Corr(t, B, GATE)
    d_in = api.DeviceArray.from_numpy(np.concatenate([x.view(np.float32), np.zeros(4 * B, np.float32)]))
    sv = np.full(K * 2 + 8, 1234.5, np.float32)
    sm = np.full(K * n + 8, 1234.5, np.float32)
    d_val, d_idx, d_m = api.DeviceArray.from_numpy(sv), api.DeviceArray.from_numpy(sv), api.DeviceArray.from_numpy(sm)
    lib = L.load()
    nb = C.c_size_t(7)

    def call(pi, n_in, pv, px, ps, pm, ms, stream=None):
        return lib.sfe_dsp_corr_process_stream(cr._h, pi, n_in, n_in, pv, px, ps, pm, ms, C.byref(nb), stream)

    good = (d_in.ptr, n, d_val.ptr, d_idx.ptr, 2, d_m.ptr, n)
    assert call(d_in.ptr, n - 1, *good[2:]) == L.SFE_EINVAL                       # n_in not a multiple of B
    assert call(d_in.ptr, n - _advance(Lt), *good[2:]) == L.SFE_EINVAL            # ... a multiple of V is not enough
    assert call(d_in.ptr, n, d_val.ptr, d_idx.ptr, 1, d_m.ptr, n) == L.SFE_ERANGE            # peak_stride too small
    assert call(d_in.ptr, n, d_val.ptr, d_idx.ptr, 2, d_m.ptr, n - 1) == L.SFE_ERANGE        # metric_stride too small
    assert call(d_in.ptr + 4, n, *good[2:]) == L.SFE_EINVAL                       # misaligned cf32 input
    assert call(d_in.ptr, n, d_val.ptr + 2, d_idx.ptr, 2, d_m.ptr, n) == L.SFE_EINVAL        # misaligned outputs
    assert call(d_in.ptr, n, d_val.ptr, d_idx.ptr + 1, 2, d_m.ptr, n) == L.SFE_EINVAL
    assert call(d_in.ptr, n, d_val.ptr, d_idx.ptr, 2, d_m.ptr + 2, n) == L.SFE_EINVAL
    assert call(d_in.ptr, n, d_in.ptr + 64, d_idx.ptr, 2, d_m.ptr, n) == L.SFE_EINVAL        # an output overlaps the input
    assert call(d_in.ptr, n, d_val.ptr, d_in.ptr + 8 * n - 4, 2, d_m.ptr, n) == L.SFE_EINVAL
    assert call(d_in.ptr, n, d_val.ptr, d_idx.ptr, 2, d_in.ptr + 128, n) == L.SFE_EINVAL
    assert call(None, n, *good[2:]) == L.SFE_EINVAL                               # null buffers
    assert call(d_in.ptr, n, None, d_idx.ptr, 2, d_m.ptr, n) == L.SFE_EINVAL
    assert call(d_in.ptr, n, d_val.ptr, None, 2, d_m.ptr, n) == L.SFE_EINVAL
    assert nb.value == 0
    assert lib.sfe_dsp_corr_set_input_format(cr._h, 7) == L.SFE_EINVAL            # a bad format: the handle stays cf32
    assert lib.sfe_dsp_corr_set_input_format(cr._h, L.FMT_TX10) == L.SFE_EINVAL
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
        rc = call(*good, s.value)
    finally:
        g = C.c_void_p()
        hip.hipStreamEndCapture(s, C.byref(g))
    if g.value:
        hip.hipGraphDestroy(g)
    hip.hipStreamDestroy(s)
    assert rc == L.SFE_ESTATE and nb.value == 0
    api.sync()
    assert np.array_equal(d_val.to_numpy(), sv) and np.array_equal(d_idx.to_numpy(), sv) and np.array_equal(d_m.to_numpy(), sm)
    assert np.array_equal(d_in.to_numpy(2 * n), x.view(np.float32))
    # nothing advanced either: the next good call is a fresh handle's
    assert call(*good) == 0 and nb.value == 2
    fresh = _run(api, api.Corr(t, B, GATE), x[None, :], [n])
    assert np.array_equal(_bits(d_val.to_numpy(K * 2)), _bits(fresh[0].ravel()))
    assert np.array_equal(d_idx.to_numpy(K * 2).view(np.uint32), fresh[1].ravel())
    assert np.array_equal(_bits(d_m.to_numpy(K * n)), _bits(fresh[2].ravel()))
    assert np.abs(fresh[2][0] - _case(Lt, n, 0)[1][:K]).max() <= TOL
