"""The streaming spatial covariance estimator on the GPU (sfe_dsp_cov_*, csrc/cov.hip) against the float64 reference of
its law (synth.cov_reference), and the parts of the contract that are about bits: any cut of the stream at a chunk, either
input format, bands against one-band handles, subsets of the streams, symmetry, exact integer Grams, where a NaN goes,
run-to-run determinism, reset, addresses and strides, the refusals; then the loop the block closes (cov -> MVDR weights
-> beam) and the layout it shares with the channelizer.

The accuracy bar is derived, not measured.  Every output float is a float32 sum nested d = T + C + ceil(A / (T C)) + 1
deep (a chunk's fmaf chain, the fold of a group's chunks, the fold of a row's groups, the scale), so it errs by at most
d 2^-24 |scale| sum_m |u_i[m] u_j[m]| to first order.  The reference is rounded to float32 for the comparison, which
costs it one more rounding of the result (covered by the factor 2):

    |G - ref| <= 2 d 2^-24 |scale| sum_m |u_i[m] u_j[m]| + 1e-30        per output float

The shapes are the smallest at which the kernel can still go wrong: S = 8 is one full tile of 16 rows, 9 the first padded
second tile, 33 and 64 the four-wave classes; A / T = 5 and 17 sit just past C = 2 and C = 4, so a short last group
exists.  The input is the synthetic stream (multiples of 2^-23 in [-1, 1)) or uniformly random (I,Q) bytes."""
import ctypes as C

import numpy as np
import pytest

from simplefe_amd import synth

pytestmark = pytest.mark.gpu
T = 64
PARITY_S = [1, 2, 3, 8, 9, 33, 64]
PARITY_A = [T, 2 * T, 5 * T, 17 * T]
NMAX = 3 * max(PARITY_A) + 2 * T
MARGIN = 4096                   # guard bytes on both sides of every row
SENT = np.float32(-7654.25)
NAN_BYTES = np.array([0x7fc00001, 0xffc12345, 0x7f800001, 0xffffffff], np.uint32).tobytes()
FF_BYTES = b"\xff"
SENT_BYTES = np.array([SENT], np.float32).tobytes()


@pytest.fixture(scope="module")
def api():
    from simplefe_amd import api as a
    assert a.cov_plan(1, 1, T)[0] == T
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
                       ("hipStreamDestroy", [C.c_void_p]), ("hipGraphGetNodes", [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)])):
        fn = getattr(h, name)
        fn.argtypes, fn.restype = args, C.c_int
    return h


_inputs = {}


def _input(S, M, n, u8):
    """(what is uploaded, the same as complex64), (S, M, n): the synthetic stream, or random bytes and their conversion.
    Computed once per key and left unchanged."""
    key = (S, M, n, u8)
    if key not in _inputs:
        if u8:
            b = synth.offset_bytes(S * M * n, seed=synth.SEED + 11 * S + M).reshape(S, M, 2 * n)
            _inputs[key] = (b, synth.u8_to_cf32(b.reshape(-1)).reshape(S, M, n))
        else:
            x = np.stack([synth.synth_cf32(M * n, ch=s).view(np.complex64).reshape(M, n) for s in range(S)])
            _inputs[key] = (x, x)
    return _inputs[key]


def _bits(y):
    return np.ascontiguousarray(y).view(np.uint32)


def _depth(api, S, M, A):
    t, c = api.cov_plan(S, M, A)
    return t + c + -(-A // (t * c)) + 1


def _bound(api, x, S, M, A, scale):
    """The per-float bound of the module's docstring for the rows x (S, M, n) completes: (M, rows, 2S, 2S) float64."""
    U = np.abs(synth.cov_columns(x, S, M))
    rows = U.shape[2] // A
    U = U[:, :, :rows * A].reshape(M, 2 * S, rows, A)
    return 2.0 * _depth(api, S, M, A) * 2.0 ** -24 * abs(scale) * np.einsum("kira,kjra->krij", U, U) + 1e-30


def _check(tag, got, ref, bound):
    """got (M, rows, 2S, 2S) float32 against ref float64, rounded to float32 for the comparison; contract 5 on the way."""
    assert got.shape == ref.shape and got.dtype == np.float32, (tag, got.shape, ref.shape)
    g, r = got.astype(np.float64), ref.astype(np.float32).astype(np.float64)
    err = np.abs(g - r)
    worst = float((err / bound).max())
    print("cov %s: worst error %.3f of its bound" % (tag, worst))
    assert np.isfinite(g).all(), tag
    assert (err <= bound).all(), (tag, worst)
    assert np.array_equal(_bits(got), _bits(got.transpose(0, 1, 3, 2))), tag         # G[i][j] and G[j][i]: the same bits
    return worst


def _run(api, cov, up, cuts, u8=False):
    """The calls `cuts` (instants each) over one input buffer (S M rows of sum(cuts)): (rows (M, rows, 2S, 2S), n_rows of
    every call, True when every call that completed no row left the sentinel-filled output as it was)."""
    n, n2 = sum(cuts), 2 * cov.n_in
    gram, most = n2 * n2, -(-sum(cuts) // cov.n_avg) + 1
    d_in = api.DeviceArray.from_bytes(up) if u8 else api.DeviceArray.from_numpy(np.ascontiguousarray(up).view(np.float32))
    image = np.full(cov.n_bands * most * gram, SENT, np.float32)
    d_out = api.DeviceArray.from_numpy(image)
    counts, at, done, untouched = [], 0, 0, True
    try:
        for m in cuts:
            k = cov.process_stream(d_in.ptr + at * (2 if u8 else 8), m, d_out.ptr + done * gram * 4, in_stride=n, out_stride=most * gram)
            counts.append(k)
            if k == 0:
                api.sync()
                untouched = untouched and np.array_equal(_bits(d_out.to_numpy()), _bits(image))
            else:
                image = d_out.to_numpy()
            at, done = at + m, done + k
        got = d_out.to_numpy().reshape(cov.n_bands, most, n2, n2)
    finally:
        d_in.free()
        d_out.free()
    assert (_bits(got[:, done:]) == _bits(SENT)).all()
    return np.ascontiguousarray(got[:, :done]), counts, untouched


@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("S", PARITY_S)
def test_accuracy_against_float64(api, L, S, M):
    """Three rows and an unfinished one (with A = T, where every call ends on a row, a fourth), both formats."""
    worst = 0.0
    for A in PARITY_A:
        n, scale = 3 * A + T, 1.0 / A
        cov = api.Cov(S, M, A, scale)
        for u8 in (False, True):
            cov.set_input_format(L.FMT_U8 if u8 else L.FMT_F32)
            cov.reset()
            up, x = _input(S, M, NMAX, u8)
            up, x = np.ascontiguousarray(up[:, :, :(2 if u8 else 1) * n]), np.ascontiguousarray(x[:, :, :n])
            got = cov.gram(up)
            assert got.shape[1] == n // A
            worst = max(worst, _check("S=%d M=%d A=%d %s" % (S, M, A, "u8" if u8 else "cf32"), got, synth.cov_reference(x, S, M, A, scale),
                                      _bound(api, x, S, M, A, scale)))
        cov.close()
    print("cov S=%d M=%d: worst error over A and formats %.3f of its bound" % (S, M, worst))


def test_any_cut_at_a_chunk_gives_the_same_rows(api):
    """Contract 1.  A = 17 T: groups of 8, 8 and 1 chunks.  53 chunks in one call, then cut at [1, 2, 3, 5, rest] chunks
    (mid-group and mid-row), then at group ends (8, 16, 42) and row ends (17, 34)."""
    S, M, A = 9, 3, 17 * T
    assert api.cov_plan(S, M, A) == (T, 8)
    n = 3 * A + 2 * T
    _, x = _input(S, M, NMAX, False)
    x = np.ascontiguousarray(x[:, :, :n])
    cov = api.Cov(S, M, A, 1.0 / A)
    one, counts, _ = _run(api, cov, x, [n])
    assert counts == [3]
    _check("one call S=9 M=3 A=17T", one, synth.cov_reference(x, S, M, A, 1.0 / A), _bound(api, x, S, M, A, 1.0 / A))
    for chunks, want in (([1, 2, 3, 5, 42], [0, 0, 0, 0, 3]), ([8, 8, 1, 17, 8, 11], [0, 0, 1, 1, 0, 1]), ([1] * 53, None)):
        cov.reset()
        cut, counts, untouched = _run(api, cov, x, [c * T for c in chunks])
        if want is None:
            want = [1 if (i + 1) % 17 == 0 else 0 for i in range(53)]
        assert counts == want, (chunks, counts)
        assert untouched, chunks
        assert np.array_equal(_bits(cut), _bits(one)), chunks
    cov.close()


def test_u8_gives_the_bits_of_cf32_and_a_band_is_a_one_band_handle(api, L):
    """Contracts 2 and 3.  The format is switched in mid-row (and mid-group) on one handle: the carried state is sums."""
    S, M, A = 9, 3, 5 * T
    n = 2 * A
    up, x = _input(S, M, NMAX, True)
    up, x = np.ascontiguousarray(up[:, :, :2 * n]), np.ascontiguousarray(x[:, :, :n])
    ref = api.Cov(S, M, A, 1.0 / A).gram(x)
    assert ref.shape == (M, 2, 2 * S, 2 * S) and np.abs(ref).max() > 0
    cov = api.Cov(S, M, A, 1.0 / A)
    cov.set_input_format(L.FMT_U8)
    assert np.array_equal(_bits(cov.gram(up)), _bits(ref))
    # 3 T instants as bytes, the other 7 T as cf32, over the same output
    cov.reset()
    n2, cutat = 2 * S, 3 * T
    d_b, d_f = api.DeviceArray.from_bytes(up), api.DeviceArray.from_numpy(x.view(np.float32))
    d_out = api.DeviceArray(M * 2 * n2 * n2)
    assert cov.process_stream(d_b, cutat, d_out, in_stride=n, out_stride=2 * n2 * n2) == 0
    cov.set_input_format(L.FMT_F32)
    assert cov.process_stream(d_f.ptr + cutat * 8, n - cutat, d_out, in_stride=n, out_stride=2 * n2 * n2) == 2
    assert np.array_equal(_bits(d_out.to_numpy().reshape(ref.shape)), _bits(ref))
    for d in (d_b, d_f, d_out):
        d.free()
    for k in range(M):
        alone = api.Cov(S, 1, A, 1.0 / A).gram(np.ascontiguousarray(x[:, k]))
        assert np.array_equal(_bits(alone[0]), _bits(ref[k])), k
        for k2 in range(k):
            assert not np.array_equal(ref[k], ref[k2])              # the band index is not ignored


def test_an_entry_depends_on_its_two_rows_only(api):
    """Contract 4: nine S = 1 handles give the 2 x 2 diagonal blocks, an S = 2 handle over streams (0, 8) the entries
    across the tile boundary."""
    S, M, A = 9, 1, 5 * T
    n = 2 * A + T
    _, x = _input(S, M, NMAX, False)
    x = np.ascontiguousarray(x[:, :, :n])
    full = api.Cov(S, M, A, 0.125).gram(x)[0]                           # (2, 18, 18)
    for s in range(S):
        alone = api.Cov(1, 1, A, 0.125).gram(np.ascontiguousarray(x[s]))[0]
        assert np.array_equal(_bits(alone), _bits(full[:, 2 * s:2 * s + 2, 2 * s:2 * s + 2])), s
    pair = api.Cov(2, 1, A, 0.125).gram(np.ascontiguousarray(x[[0, 8]]))[0]
    pick = [0, 1, 16, 17]
    assert np.array_equal(_bits(pair), _bits(full[:, pick][:, :, pick]))
    assert np.abs(pair[:, :2, 2:]).min() > 0


@pytest.mark.parametrize("scale", [1.0, 0.5])
def test_small_integers_give_the_exact_gram(api, scale):
    """Contract 6, and the layout test: with an asymmetric integer input a transposed tile, a swapped lane or a wrong
    mirror cannot pass it."""
    S, M, A = 9, 2, 64 * T
    rng = np.random.default_rng(6)
    v = rng.integers(-8, 9, (S, M, 2 * A, 2))
    x = (v[..., 0] + 1j * v[..., 1]).astype(np.complex64)
    got = api.Cov(S, M, A, scale).gram(x)
    u = v.transpose(1, 0, 3, 2).reshape(M, 2 * S, 2, A).astype(np.int64)           # (M, 2S, rows, A)
    want = np.einsum("kira,kjra->krij", u, u)
    assert got.shape == want.shape == (M, 2, 2 * S, 2 * S)
    assert np.array_equal(got.astype(np.float64), scale * want.astype(np.float64))
    assert not np.array_equal(want[:, 0], want[:, 1])


def test_a_nan_poisons_its_own_stream_band_and_row(api):
    """Contract 7: rows and columns 6 and 7 of band 1, output row 1, and nothing else; padding rows multiply 0 by 0."""
    S, M, A = 9, 3, 5 * T
    n = 3 * A
    _, x = _input(S, M, NMAX, False)
    x = np.ascontiguousarray(x[:, :, :n])
    clean = api.Cov(S, M, A, 1.0 / A).gram(x)
    bad = x.copy()
    bad[3, 1, A + 2 * T + 5] = complex(np.nan, np.nan)
    got = api.Cov(S, M, A, 1.0 / A).gram(bad)
    hit = np.zeros(got.shape, bool)
    hit[1, 1, 6:8, :] = True
    hit[1, 1, :, 6:8] = True
    assert np.isfinite(clean).all()
    assert not np.isfinite(got[hit]).any()
    assert np.isfinite(got[~hit]).all() and np.array_equal(_bits(got[~hit]), _bits(clean[~hit]))


def test_the_same_call_gives_the_same_bits(api):
    S, M, A = 33, 2, 17 * T
    _, x = _input(S, M, NMAX, False)
    x = np.ascontiguousarray(x[:, :, :2 * A + T])
    cov = api.Cov(S, M, A, 1.0 / A)
    runs = []
    for _ in range(3):
        cov.reset()
        runs.append(_bits(cov.gram(x)))
    assert runs[0].shape[1] == 2 and np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], runs[2])


def test_reset_makes_a_fresh_handle(api):
    S, M, A = 9, 2, 17 * T
    _, x = _input(S, M, NMAX, False)
    a, b = np.ascontiguousarray(x[:, :, :9 * T]), np.ascontiguousarray(x[:, :, 9 * T:9 * T + A])
    cov = api.Cov(S, M, A, 1.0 / A)
    assert cov.gram(a).shape[1] == 0                    # an open row, an open group
    cov.reset()
    first = cov.gram(b)
    fresh = api.Cov(S, M, A, 1.0 / A).gram(b)
    assert first.shape[1] == 1 and np.array_equal(_bits(first), _bits(fresh))


class Rows:
    """A device buffer of `rows` rows of n elements of `esz` bytes, the first `shift` elements behind a guard, with at
    least MARGIN guard bytes in front of every row and behind the last (the stride is n + extra + the guard); guards and
    gaps hold the repeated `fill_bytes` pattern."""

    def __init__(self, api, rows, n, esz, fill_bytes, extra=0, shift=0):
        self.api, self.rows, self.n, self.esz = api, rows, n, esz
        self.stride = n + extra + -(-MARGIN // esz)
        self.off = MARGIN + shift * esz
        self.nbytes = -(-(self.off + rows * self.stride * esz + MARGIN) // 4) * 4
        self.host = np.frombuffer(np.resize(np.frombuffer(fill_bytes, np.uint8), self.nbytes).tobytes(), np.uint8).copy()
        self.d = api.DeviceArray(self.nbytes // 4)
        self.ptr = self.d.ptr + self.off

    def payload(self):
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
        lo, hi = self.off, self.off + self.rows * self.stride * self.esz
        body, wbody = got[lo:hi].reshape(self.rows, -1), self.host[lo:hi].reshape(self.rows, -1)
        intact = (np.array_equal(got[:lo], self.host[:lo]) and np.array_equal(got[hi:], self.host[hi:])
                  and np.array_equal(body[:, self.n * self.esz:], wbody[:, self.n * self.esz:]))
        return body[:, :self.n * self.esz].copy(), intact

    def free(self):
        self.d.free()


@pytest.mark.parametrize("u8", [False, True], ids=["cf32", "u8"])
def test_any_address_and_stride_gives_the_same_bits(api, L, u8):
    """The same data 1, 2 and 3 samples into larger buffers with other strides (u8: an odd 2-byte offset at shift 1 and
    3), NaN bit patterns (bytes 0xFF for u8) all around every input row, a sentinel all around every output row."""
    S, M, A = 9, 3, 5 * T
    n = 2 * A + T
    up, x = _input(S, M, NMAX, u8)
    up = np.ascontiguousarray(up[:, :, :(2 if u8 else 1) * n])
    cov = api.Cov(S, M, A, 1.0 / A)
    cov.set_input_format(L.FMT_U8 if u8 else L.FMT_F32)
    one = cov.gram(up)
    gram = 4 * S * S
    for shift in (1, 2, 3):
        cov.reset()
        src = Rows(api, S * M, n, 2 if u8 else 8, FF_BYTES if u8 else NAN_BYTES, shift + 2, shift).upload(up)
        dst = Rows(api, M, 2 * gram, 4, SENT_BYTES, 7 - shift, 4 - shift).upload(np.full((M, 2 * gram), SENT, np.float32))
        try:
            assert cov.process_stream(src.ptr, n, dst.ptr, in_stride=src.stride, out_stride=dst.stride) == 2
            api.sync()
            pay, intact = dst.download()
            _, in_intact = src.download()
        finally:
            src.free()
            dst.free()
        assert intact and in_intact, shift
        assert np.array_equal(pay.view(np.uint32).reshape(M, 2, 2 * S, 2 * S), _bits(one)), shift
    cov.close()


def test_refusals_launch_nothing(api, L, hip):
    S, M, A = 3, 2, 2 * T
    n, gram = 2 * A, 4 * S * S
    _, x = _input(S, M, NMAX, False)
    x = np.ascontiguousarray(x[:, :, :n])
    cov = api.Cov(S, M, A, 1.0)
    d_in = api.DeviceArray.from_numpy(np.concatenate([x.view(np.float32).ravel(), np.zeros(64, np.float32)]))
    sentinel = np.full(M * 2 * gram + 64, SENT, np.float32)
    d_out = api.DeviceArray.from_numpy(sentinel)
    lib = L.load()
    k = C.c_size_t(7)
    os_ = 2 * gram

    def call(pi, n_in, in_stride, po, out_stride, stream=None, h=None):
        return lib.sfe_dsp_cov_process_stream(h or cov._h, pi, n_in, in_stride, po, out_stride, C.byref(k), stream)

    assert call(d_in.ptr, n, n, d_out.ptr, os_ - 1) == L.SFE_ERANGE                  # out_stride one float short of two rows
    assert call(d_in.ptr, n, n, d_in.ptr + 8 * 16, os_) == L.SFE_EINVAL              # output overlaps input
    assert call(d_in.ptr + 4, n, n, d_out.ptr, os_) == L.SFE_EINVAL                  # misaligned cf32 input
    assert call(d_in.ptr, n, n, d_out.ptr + 2, os_) == L.SFE_EINVAL                  # misaligned output
    assert call(d_in.ptr, n, n - 1, d_out.ptr, os_) == L.SFE_EINVAL                  # in_stride one sample short
    assert call(None, n, n, d_out.ptr, os_) == L.SFE_EINVAL                          # null input
    assert call(d_in.ptr, n, n, None, os_) == L.SFE_EINVAL                           # null output
    assert call(d_in.ptr, n - 1, n, d_out.ptr, os_) == L.SFE_EINVAL                  # not a multiple of the chunk
    assert call(d_in.ptr, T // 2, n, d_out.ptr, os_) == L.SFE_EINVAL
    assert call(d_in.ptr, 1 << 31, 1 << 31, d_out.ptr, 1 << 31) == L.SFE_EINVAL      # 2^31 instants
    assert lib.sfe_dsp_cov_process_stream(cov._h, d_in.ptr, n, n, d_out.ptr, os_, None, None) == L.SFE_EINVAL       # no counter
    cov.set_input_format(L.FMT_U8)
    assert call(d_in.ptr + 1, n, n, d_out.ptr, os_) == L.SFE_EINVAL                  # an odd u8 address
    cov.set_input_format(L.FMT_F32)
    assert lib.sfe_dsp_cov_set_input_format(cov._h, 7) == L.SFE_EINVAL               # a bad format: the handle stays cf32
    assert lib.sfe_dsp_cov_set_input_format(cov._h, L.FMT_TX10) == L.SFE_EINVAL
    assert k.value == 0
    assert call(d_in.ptr, 0, 0, d_out.ptr, 0) == L.SFE_OK and k.value == 0           # n_in = 0: a no-op
    # a capturing stream: refused, and the capture ends as an empty graph
    s = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(s)) == 0
    assert hip.hipStreamBeginCapture(s, 2) == 0            # relaxed mode: the refused call launches nothing
    try:
        rc = call(d_in.ptr, n, n, d_out.ptr, os_, s.value)
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
    # a live handle of another block is refused by every cov function, and cov's destroy frees nothing of it
    other = api.Iir(synth.iir_dc_blocker(0.995))
    assert call(d_in.ptr, n, n, d_out.ptr, os_, h=other._h) == L.SFE_EINVAL and k.value == 0
    assert lib.sfe_dsp_cov_set_input_format(other._h, L.FMT_F32) == L.SFE_EINVAL
    assert lib.sfe_dsp_cov_reset(other._h) == L.SFE_EINVAL
    assert lib.sfe_dsp_cov_destroy(other._h) == L.SFE_OK
    blk = other.block
    assert np.isfinite(other.filter(x[0, 0, :blk])).all()                           # still alive
    assert lib.sfe_dsp_iir_process_stream(cov._h, d_in.ptr, blk, blk, d_out.ptr, blk, C.byref(k), None) == L.SFE_EINVAL
    api.sync()
    assert np.array_equal(d_out.to_numpy(), sentinel)
    assert np.array_equal(d_in.to_numpy(x.size * 2), x.view(np.float32).ravel())
    # the next good call is a fresh handle's: no refusal moved the counter
    assert cov.process_stream(d_in, n, d_out, out_stride=os_) == 2
    got = d_out.to_numpy(M * os_).reshape(M, 2, 2 * S, 2 * S)
    assert np.array_equal(_bits(got), _bits(api.Cov(S, M, A, 1.0).gram(x)))
    assert np.array_equal(d_out.to_numpy()[M * os_:], sentinel[M * os_:])
    d_in.free()
    d_out.free()


def _sir_db(y_d, y_i):
    return 10.0 * np.log10((np.abs(y_d.astype(np.complex128)) ** 2).sum() / (np.abs(y_i.astype(np.complex128)) ** 2).sum())


def test_cov_mvdr_beam_closes_the_loop(api):
    """Cov -> cov_from_gram -> mvdr_weights -> Beam on a scene with an interferer 30 dB above the signal.  One wrong Gram
    entry costs tens of dB; the 1 dB is not a measurement of the kernel."""
    S, n = 4, 4096
    x, x_d, x_i, a = synth.cov_scene(S, n, 7)
    sir_in = _sir_db(x_d, x_i)
    # the float64 chain
    C64, _ = synth.cov_from_gram(synth.cov_reference(x, S, 1, n, 1.0 / n)[0, 0])
    w64 = synth.mvdr_weights(C64, a, 1e-6)[0, 0].astype(np.complex128)
    sir_ref = _sir_db(w64 @ x_d.astype(np.complex128), w64 @ x_i.astype(np.complex128))
    # the GPU chain
    G = api.Cov(S, 1, n, 1.0 / n).gram(x)
    assert G.shape == (1, 1, 2 * S, 2 * S)
    Cg, _ = synth.cov_from_gram(G[0, 0])
    beam = api.Beam(synth.mvdr_weights(Cg, a, 1e-6))
    sir_gpu = _sir_db(beam.mix(x_d), beam.mix(x_i))
    print("cov -> mvdr -> beam: SIR in %.1f dB, float64 chain %.2f dB, GPU chain %.2f dB" % (sir_in, sir_ref, sir_gpu))
    assert abs(sir_in + 30.0) < 0.5
    assert sir_ref >= 40.0
    assert abs(sir_gpu - sir_ref) <= 1.0


def test_chan_cov_share_their_layout(api):
    """chan -> cov over one device buffer with no copy between them: chan's output rows (s M + k) are cov's input rows."""
    M, D, S = 16, 8, 2
    n = 8192
    no, A = n // D, 4 * T
    h = synth.lowpass_taps(16 * M + 1, 2.0 / M)
    x = np.stack([synth.synth_cf32(n, ch=20 + s).view(np.complex64) for s in range(S)])
    chan, cov = api.Chan(h, M, D, n_streams=S), api.Cov(S, M, A, 1.0 / A)
    d_x = api.DeviceArray.from_numpy(x.view(np.float32))
    d_c, d_g = api.DeviceArray(S * M * no * 2), api.DeviceArray(M * (no // A) * 4 * S * S)
    assert chan.process_stream(d_x, n, d_c, out_stride=no) == no
    assert cov.process_stream(d_c, no, d_g, in_stride=no) == no // A
    got = d_g.to_numpy().reshape(M, no // A, 2 * S, 2 * S)
    mid = d_c.to_numpy().view(np.complex64).reshape(S, M, no)                       # what the channelizer actually wrote
    for d in (d_x, d_c, d_g):
        d.free()
    bound = _bound(api, mid, S, M, A, 1.0 / A)
    _check("cov of chan's own output", got, synth.cov_reference(mid, S, M, A, 1.0 / A), bound)
    X = np.stack([synth.chan_reference(x[s], h, M, D) for s in range(S)])          # (S, M, no)
    _check("chan -> cov against the two references composed", got, synth.cov_reference(X, S, M, A, 1.0 / A), bound)
    assert np.abs(got).max() > 1e-6
