"""The streaming Welch spectrum estimator on the GPU (sfe_dsp_psd_*, csrc/psd.hip) against the float64 reference of its
contract (synth.psd_reference: frame, window, np.fft.fft, squared magnitude, sum), and the parts of the contract that
are about bits: any cut of the stream, either input format, reset and refusals.  `-m gpu`.

TOL is the project's parity bar for every bank.  A float32 emulation of this law in numpy against float64 on these
inputs gives 6e-8 to 3e-7 rel-RMS and 4e-7 to 1.1e-6 worst bin (N up to 4096, A up to 300): the bar has a margin of
10x to 30x over float32 itself."""
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


def _hann(N):
    return np.hanning(N).astype(np.float32)


def _errors(got, ref):
    """(rel-RMS over the bins, worst bin error over the row's RMS) of one row."""
    err = got.astype(np.float64) - ref
    rms = np.sqrt(np.mean(ref ** 2))
    return np.sqrt(np.mean(err ** 2)) / rms, np.abs(err).max() / rms


def _run_calls(api, ps, x, cuts, rows_cap):
    """Feed (n_streams, n) complex64 x to handle ps in calls of the given sizes (samples); the rows land consecutively.
    Returns (n_streams, rows, N) float32."""
    S, n = x.shape
    N = ps.n_fft
    d_in = api.DeviceArray.from_numpy(x.view(np.float32))
    d_out = api.DeviceArray(S * rows_cap * N)
    pos = rows = 0
    for c in cuts:
        k = ps.process_stream(d_in.ptr + 8 * pos, c, d_out.ptr + 4 * N * rows, in_stride=n, out_stride=rows_cap * N)
        rows += k
        pos += c
    assert pos == n
    y = d_out.to_numpy().reshape(S, rows_cap, N)[:, :rows].copy()
    d_in.free()
    d_out.free()
    return y


def _cut(total, step):
    return [step] * (total // step) + ([total % step] if total % step else [])


@pytest.mark.timeout(300)
@pytest.mark.parametrize("n_streams", [1, 3])
@pytest.mark.parametrize("A", [1, 5, 37])
@pytest.mark.parametrize("hop_of", ["N", "N/2", "3N/8+1"])
@pytest.mark.parametrize("N", [256, 1024, 4096])
def test_parity_grid(api, N, hop_of, A, n_streams):
    H = {"N": N, "N/2": N // 2, "3N/8+1": 3 * N // 8 + 1}[hop_of]
    w = _hann(N)
    scale = 1.0 / (A * float(np.sum(w.astype(np.float64) ** 2)))
    n = (2 * A + 3) * H                     # two rows complete, a third stays open (A = 1: every segment is a row, five complete)
    rows = (2 * A + 3) // A
    assert rows == (5 if A == 1 else 2)
    x = _streams(n, n_streams)
    ps = api.Psd(w, H, A, scale=scale, n_streams=n_streams)
    d_in = api.DeviceArray.from_numpy(x.view(np.float32))
    sentinel = np.full(n_streams * (rows + 1) * N, -77.0, np.float32)
    d_out = api.DeviceArray.from_numpy(sentinel)
    assert ps.process_stream(d_in, n, d_out, out_stride=(rows + 1) * N) == rows
    y = d_out.to_numpy().reshape(n_streams, rows + 1, N)
    assert np.array_equal(y[:, rows], sentinel.reshape(n_streams, rows + 1, N)[:, rows])    # the memory after the last row is untouched
    for s in range(n_streams):
        ref = synth.psd_reference(x[s], w, H, A, np.float32(scale))
        assert ref.shape == (rows, N)
        for r in range(rows):
            rel, worst = _errors(y[s, r], ref[r])
            print("psd parity N=%d H=%d A=%d s=%d row %d: rel-RMS %.2e worst bin %.2e" % (N, H, A, s, r, rel, worst))
            assert rel <= TOL and worst <= TOL, (N, H, A, s, r, rel, worst)
    ps.close()
    d_in.free()
    d_out.free()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("N, H, A, irregular", [
    # C = 8, a row's chunks hold 8, 8, 8, 8, 5 segments: inside a chunk (3), on a chunk edge (8), inside a row (28),
    # on a row edge (37), on a chunk edge of a later row (82), one segment, across two rows
    (1024, 384, 37, [3, 5, 20, 9, 45, 1, 60]),
    # C = 4, chunks of 4 and 1: inside a chunk (2), on a chunk edge (4), on a row edge (5), inside a row (8), across rows
    (4096, 4096, 5, [2, 2, 1, 3, 13, 1]),
    # C = 2, a chunk is a whole row (no row fold), four segments to a batch of the N = 256 kernel: inside a row, on row edges
    (256, 97, 2, [1, 2, 3, 1, 4, 2]),
    # the two sizes whose first pass is the radix-2 one; N = 512 has two segments to a batch.  C = 8 and C = 4 as above
    (512, 201, 37, [3, 5, 20, 9, 45, 1, 60]),
    (2048, 2048, 5, [2, 2, 1, 3, 13, 1]),
])
def test_cutting_the_stream_gives_the_same_bits(api, N, H, A, irregular):
    assert api.psd_plan(N, H, A)[0] == {37: 8, 5: 4, 2: 2}[A]
    segs = 4 * A + 11
    w = _hann(N)
    x = _streams(segs * H, 1)
    rows = segs // A                        # 4 and a row left open; 6 for A = 5, 9 for A = 2
    one = _run_calls(api, api.Psd(w, H, A, scale=0.37), x, [segs * H], rows)
    assert one.shape == (1, rows, N)
    ref = synth.psd_reference(x[0], w, H, A, np.float32(0.37))
    assert max(_errors(one[0, r], ref[r])[0] for r in range(rows)) <= TOL
    irregular = irregular + [segs - sum(irregular)]
    assert irregular[-1] > 0
    for cuts in (_cut(segs, 1), _cut(segs, 3), _cut(segs, 7), irregular):
        got = _run_calls(api, api.Psd(w, H, A, scale=0.37), x, [c * H for c in cuts], rows)
        assert got.shape == one.shape and np.array_equal(got.view(np.uint32), one.view(np.uint32)), (N, H, A, cuts[:8])


@pytest.mark.timeout(300)
@pytest.mark.parametrize("offset", [0, 2, 6])
@pytest.mark.parametrize("N, H, A", [(256, 97, 5), (1024, 1024, 3), (4096, 2048, 4), (512, 201, 3), (2048, 1024, 4)])
def test_u8_input_equals_converted_cf32(api, L, N, H, A, offset):
    segs = 3 * A + 2
    n = segs * H
    w = _hann(N)
    rng = np.random.default_rng(N + offset)
    b = rng.integers(0, 256, size=2 * n, dtype=np.uint8)
    lib = L.load()
    # cf32 path: the library's own converter over an aligned copy of the bytes
    d_b = api.DeviceArray.from_bytes(b)
    d_f = api.DeviceArray(2 * n)
    assert lib.sfe_dsp_rx_u8_to_f32(d_b.ptr, d_f.ptr, 2 * n, None) == 0
    ref_ps = api.Psd(w, H, A)
    d_ref = api.DeviceArray(3 * N)
    assert ref_ps.process_stream(d_f, n, d_ref) == 3
    want = d_ref.to_numpy()
    assert np.isfinite(want).all() and want.min() > 0
    # u8 path: the same bytes at `offset` bytes past a 16-byte boundary, fed in two calls
    d_u = api.DeviceArray((2 * n + offset) // 4 + 8)
    assert d_u.ptr % 16 == 0
    assert lib.sfe_dsp_memcpy_h2d(d_u.ptr + offset, b.ctypes.data, 2 * n, None) == 0
    ps = api.Psd(w, H, A)
    ps.set_input_format(L.FMT_U8)
    d_out = api.DeviceArray(3 * N)
    cut = (A + 1) * H
    k1 = ps.process_stream(d_u.ptr + offset, cut, d_out.ptr, out_stride=3 * N)
    k2 = ps.process_stream(d_u.ptr + offset + 2 * cut, n - cut, d_out.ptr + 4 * N * k1, out_stride=2 * N)
    assert (k1, k2) == (1, 2)
    assert np.array_equal(d_out.to_numpy().view(np.uint32), want.view(np.uint32)), (N, H, A, offset)
    # the format may change between two calls of one stream: cf32 first, then the bytes
    mix = api.Psd(w, H, A)
    d_out.zero()
    k1 = mix.process_stream(d_f.ptr, cut, d_out.ptr, out_stride=3 * N)
    mix.set_input_format(L.FMT_U8)
    k2 = mix.process_stream(d_u.ptr + offset + 2 * cut, n - cut, d_out.ptr + 4 * N * k1, out_stride=2 * N)
    assert (k1, k2) == (1, 2)
    assert np.array_equal(d_out.to_numpy().view(np.uint32), want.view(np.uint32)), (N, H, A, offset)
    # and spectrum() with (n, 2) bytes
    ps2 = api.Psd(w, H, A)
    ps2.set_input_format(L.FMT_U8)
    assert np.array_equal(ps2.spectrum(b.reshape(n, 2)).ravel().view(np.uint32), want.view(np.uint32))


@pytest.mark.timeout(300)
@pytest.mark.parametrize("N", [256, 1024, 4096, 512, 2048])
def test_a_tone_lands_in_its_bin(api, N):
    H, A, a, scale = N, 6, 0.375, 0.5
    # 1, N/2 - 1, N/2, N/2 + 1: the bins an even/odd mix-up in the first pass would swap
    for k0 in (3, N - 3, 1, N // 2 - 1, N // 2, N // 2 + 1):
        x = (a * np.exp(2j * np.pi * k0 * np.arange(2 * A * H) / N)).astype(np.complex64)
        rows = api.Psd(np.ones(N, np.float32), H, A, scale=scale).spectrum(x)[0]
        assert rows.shape == (2, N)
        want = scale * A * (a * N) ** 2
        for r in range(2):
            assert int(np.argmax(rows[r])) == k0, (N, k0, r)
            assert abs(float(rows[r][k0]) - want) <= 1e-5 * want, (N, k0, r, float(rows[r][k0]), want)


@pytest.mark.timeout(300)
def test_reset_and_streams_are_independent(api):
    N, H, A = 1024, 384, 7
    w = _hann(N)
    n = (3 * A + 4) * H                     # the handle is left in mid-row
    x = _streams(n, 3)
    ps = api.Psd(w, H, A, n_streams=3)
    first = ps.spectrum(_streams(n, 3, first=12345))        # something to forget
    ps.reset()
    after_reset = ps.spectrum(x)
    fresh = api.Psd(w, H, A, n_streams=3).spectrum(x)
    assert fresh.shape == (3, 3, N)
    assert np.array_equal(after_reset.view(np.uint32), fresh.view(np.uint32))
    assert not np.array_equal(first.view(np.uint32), fresh.view(np.uint32))
    for s in range(3):
        alone = api.Psd(w, H, A).spectrum(x[s])[0]
        assert np.array_equal(alone.view(np.uint32), fresh[s].view(np.uint32)), s
    assert max(_errors(fresh[1, r], synth.psd_reference(x[1], w, H, A, 1.0)[r])[0] for r in range(3)) <= TOL


def _large(api, log2n, A, rows_checked):
    """One call of 2^log2n cf32 samples from fill_synth, N = H = 1024; the named rows against float64 references built
    from those rows' samples only."""
    N = H = 1024
    n = 1 << log2n
    rows = n // H // A
    w = _hann(N)
    scale = 1.0 / (A * float(np.sum(w.astype(np.float64) ** 2)))
    d_in = api.DeviceArray(2 * n)
    d_in.fill_synth(synth.SEED)
    d_out = api.DeviceArray(rows * N)
    ps = api.Psd(w, H, A, scale=scale)
    assert ps.process_stream(d_in, n, d_out) == rows
    y = d_out.to_numpy().reshape(rows, N)
    d_in.free()
    d_out.free()
    ps.close()
    for r in rows_checked:
        xr = synth.synth_cf32(A * H, first_sample=r * A * H).view(np.complex64)
        assert synth.psd_rows(xr.size, N, H, A, first=r * A * H) == (r, r + 1)
        ref = synth.psd_reference(xr, w, H, A, np.float32(scale), first=r * A * H)[0]
        rel, worst = _errors(y[r], ref)
        print("psd large 2^%d A=%d row %d: rel-RMS %.2e worst bin %.2e" % (log2n, A, r, rel, worst))
        assert rel <= TOL and worst <= TOL, (log2n, A, r, rel, worst)


@pytest.mark.timeout(300)
def test_sixteen_rows_of_a_large_call(api):
    assert api.psd_plan(1024, 1024, 4096)[0] == 64
    _large(api, 26, 4096, (0, 7, 15))


@pytest.mark.timeout(300)
def test_one_row_over_a_whole_capture(api):
    assert api.psd_plan(1024, 1024, 16384)[0] == 128
    _large(api, 24, 16384, (0,))


@pytest.mark.timeout(300)
def test_refusals_launch_nothing(api, L):
    N, H, A = 1024, 384, 5
    w = _hann(N)
    n = (2 * A + 1) * H
    x = _streams(n, 1)
    ps = api.Psd(w, H, A)
    d_in = api.DeviceArray.from_numpy(np.concatenate([x.view(np.float32).ravel(), np.zeros(2 * N, np.float32)]))
    sentinel = np.full(2 * N, 1234.5, np.float32)
    d_out = api.DeviceArray.from_numpy(sentinel)
    lib = L.load()
    k = C.c_size_t(7)

    def call(pi, n_in, in_stride, po, out_stride, stream=None):
        return lib.sfe_dsp_psd_process_stream(ps._h, pi, n_in, in_stride, po, out_stride, C.byref(k), stream)

    assert call(d_in.ptr, n - 1, n, d_out.ptr, 2 * N) == L.SFE_EINVAL             # n_in not a multiple of H
    assert call(d_in.ptr + 4, n, n, d_out.ptr, 2 * N) == L.SFE_EINVAL             # misaligned cf32 input
    assert call(d_in.ptr, n, n, d_out.ptr + 2, 2 * N) == L.SFE_EINVAL             # misaligned output
    assert call(d_in.ptr, n, n, d_in.ptr + 8 * 16, 2 * N) == L.SFE_EINVAL         # output overlaps input
    assert call(d_in.ptr, n, n, d_out.ptr, 2 * N - 1) == L.SFE_ERANGE             # out_stride one float short
    assert call(None, n, n, d_out.ptr, 2 * N) == L.SFE_EINVAL                     # null input
    assert k.value == 0
    assert lib.sfe_dsp_psd_set_input_format(ps._h, 7) == L.SFE_EINVAL             # a bad format: the handle stays cf32
    assert lib.sfe_dsp_psd_set_input_format(ps._h, L.FMT_TX10) == L.SFE_EINVAL
    # a capturing stream: the segment counter lives on the host
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
        rc = call(d_in.ptr, n, n, d_out.ptr, 2 * N, s.value)
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
    assert ps.process_stream(d_in, n, d_out, out_stride=2 * N) == 2
    got = d_out.to_numpy().reshape(2, N)
    fresh = api.Psd(w, H, A).spectrum(x)[0]
    assert np.array_equal(got.view(np.uint32), fresh.view(np.uint32))
    ref = synth.psd_reference(x[0], w, H, A, 1.0)
    assert max(_errors(got[r], ref[r])[0] for r in range(2)) <= TOL
