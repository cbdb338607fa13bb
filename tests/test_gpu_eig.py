"""The eigen-decomposition / MUSIC direction finder on the GPU (sfe_dsp_eig_*, csrc/eig.hip) against the float64 statement
of its law (synth.eig_reference, numpy.linalg.eigh), the parts of the contract that are about bits, the device-resident
loop cov -> eig -> load_beam -> beam, and the refusals.

The accuracy bars are measured, not fixed.  For every input the test also evaluates the law in float32 through LAPACK
(numpy.linalg.eigh on the float32 G^, the null spectrum in float32 numpy) and compares both with the float64 reference of
the same float32 G.  With n = 2S, lambda_0 the largest eigenvalue and V read from the eigen-beam output with E = S:

    eigenvalues       max |d lambda| / lambda_0                      <= max(4 x LAPACK-float32's, n 2^-23)
    orthogonality     max |V^T V - I|                                <= the same form
    residual          max |G^ V - V Lambda| / lambda_0               <= the same form
    projector, null   |P_D - P_D(ref)|_F, max |d null|               <= max(4 x LAPACK-float32's, n 2^-23 / g)

g = (lambda_{D-1} - lambda_D) / lambda_0 is the relative gap behind the signal subspace, computed in float64 per input
and asserted to be >= 1e-4: the last line is the Davis-Kahan bound of a backward-stable solver.  (D = 0: the projector is
empty and g is taken as 1.)

Shapes are the smallest at which the kernel can go wrong: S = 1 (one pair, one step), 4, 9 (n / 2 = 9 pairs: ragged
against the lanes of a wave and the 256 of the block loop), 33 (66 vectors: the second slot of the null spectrum's lanes;
LDS still below 64 KB), 64 (the LDS maximum, 131 KB); B = 9 (ragged against the four waves) and 64; M = 3; two rows."""
import ctypes as C

import numpy as np
import pytest

from simplefe_amd import synth

pytestmark = pytest.mark.gpu
N_SCENE = 4096
MARGIN = 4096
SENT = np.float32(-7654.25)
SENT_BYTES = np.array([SENT], np.float32).tobytes()
NAN_BYTES = np.array([0x7fc00001, 0xffc12345, 0x7f800001, 0xffffffff], np.uint32).tobytes()
F32 = np.float32


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
                       ("hipStreamDestroy", [C.c_void_p]), ("hipGraphGetNodes", [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)])):
        fn = getattr(h, name)
        fn.argtypes, fn.restype = args, C.c_int
    return h


def _bits(y):
    return np.ascontiguousarray(y).view(np.uint32)


_grams = {}


def _gram(S, scene="cov", seed=7):
    """(G (2S, 2S) float32, the desired steering vector): the scene's float64 Gram over N_SCENE instants, rounded once.
    Computed once per key and left unchanged."""
    key = (S, scene, seed)
    if key not in _grams:
        x, _, _, a = (synth.cov_scene if scene == "cov" else synth.mvdr_scene_rectilinear)(S, N_SCENE, seed)
        U = synth.cov_columns(x, S, 1)[0]
        G = (U @ U.T / N_SCENE).astype(F32)
        G.setflags(write=False)
        _grams[key] = (G, a)
    return _grams[key]


def _steering(S, B, a_d):
    """(B, S) complex64: the scene's desired steering vector, then a sine grid of scan directions."""
    u = -1.0 + (2.0 * np.arange(B) + 1.0) / B
    st = np.exp(1j * np.pi * u[:, None] * np.arange(S)[None, :])
    st[0] = a_d
    return st.astype(np.complex64)


def _null_from(V, D, steering, dtype):
    """Step 4 of the law from an eigenvector matrix (columns, in the order of the values), in `dtype`."""
    N = V[:, D:].astype(dtype)
    out = np.empty(steering.shape[0], dtype)
    for b, a in enumerate(steering):
        P = N.T @ synth.mvdr_rhs(a, dtype=dtype)
        q00, q11, q01 = P[:, 0] @ P[:, 0], P[:, 1] @ P[:, 1], P[:, 0] @ P[:, 1]
        half = dtype(0.5)
        lmin = half * (q00 + q11) - np.sqrt((half * (q00 - q11)) ** 2 + q01 * q01, dtype=dtype)
        out[b] = max(lmin, dtype(0)) / dtype((np.abs(a.astype(np.complex128)) ** 2).sum())
    return out


def _proj(V, D):
    return V[:, :D] @ V[:, :D].T


def _measures(G64, lam, V, nul, D, ref):
    """(eigenvalue, orthogonality, residual, projector, null) errors of one decomposition against the float64 one."""
    lr, Vr, nr = ref
    l0, n = np.abs(lr).max(), lam.size
    lam, V = lam.astype(np.float64), V.astype(np.float64)
    return (np.abs(lam - lr).max() / l0, np.abs(V.T @ V - np.eye(n)).max(), np.abs(G64 @ V - V * lam).max() / l0,
            np.linalg.norm(_proj(V, D) - _proj(Vr, D)), np.abs(nul.astype(np.float64) - nr).max() if nr.size else 0.0)


def _check_problem(tag, G, steering, wl, D, val, nul, vec, status, gap_check=True):
    """One problem against the bars of the module's docstring; returns the worst ratio to its bar."""
    n = G.shape[0]
    lr, nr, _, sr, Vr = synth.eig_reference(G, steering, wl, D, 0)
    lr, nr, Vr = lr[0], nr[0], Vr[0]
    assert sr[0] == 0 and status == 0, (tag, status)
    assert np.isfinite(val).all() and np.isfinite(nul).all() and np.isfinite(vec).all(), tag
    assert (np.diff(val) <= 0).all(), tag
    G64 = synth.mvdr_loaded_matrix(G, wl)
    l0 = np.abs(lr).max()
    g = (lr[D - 1] - lr[D]) / l0 if D else 1.0
    if gap_check:
        assert g >= 1e-4, (tag, g)
    l32, V32 = np.linalg.eigh(synth.mvdr_loaded_matrix(G, wl, dtype=F32))
    l32, V32 = l32[::-1], V32[:, ::-1]
    lap = _measures(G64, l32, V32, _null_from(V32, D, steering, F32), D, (lr, Vr, nr))
    got = _measures(G64, val, vec.T, nul, D, (lr, Vr, nr))
    floor = n * 2.0 ** -23
    bars = [max(4.0 * lap[i], floor) for i in range(3)] + [max(4.0 * lap[i], floor / g) for i in (3, 4)]
    if not gap_check:
        got, bars = got[:3], bars[:3]
    ratio = max(e / b for e, b in zip(got, bars))
    print("eig %s g %.1e: %s: %.2f of the bar" % (tag, g, " ".join("%.1e/%.1e" % (e, b) for e, b in zip(got, bars)), ratio))
    assert all(e <= b for e, b in zip(got, bars)), (tag, got, bars)
    assert (nul >= 0).all() and (nul <= 1.0 + floor).all(), tag
    if not wl:          # contract 5: the exact W-only structure
        assert np.array_equal(_bits(vec[1::2, 0::2]), _bits(-vec[0::2, 1::2])) and np.array_equal(_bits(vec[1::2, 1::2]), _bits(vec[0::2, 0::2])), tag
    return ratio


ACC_SB = [(1, 9), (4, 64), (9, 9), (9, 64), (33, 64), (64, 9), (64, 64)]


@pytest.mark.parametrize("S,B", ACC_SB, ids=["S%d-B%d" % sb for sb in ACC_SB])
def test_accuracy_against_float64(api, S, B):
    """M = 3 bands of two rows each, six problems per call, E = S.  Linear mode, D = 4: cov_scene draws 7 .. 9 and the
    rectilinear scene's draws 7 .. 9.  Widely linear: cov_scene's three with D = 4 (row 1: the next band's matrix), then
    the rectilinear scene's three with D = 3.  S = 1: D = 0, and null is 1."""
    M, rows, n = 3, 2, 2 * S
    cov, rect = [_gram(S, "cov", 7 + i) for i in range(3)], [_gram(S, "rect", 7 + i) for i in range(3)]
    worst = 0.0
    for wl, D, ins in ((False, 4, [cov[0], rect[0], cov[1], rect[1], cov[2], rect[2]]),
                       (True, 4, [cov[0], cov[1], cov[1], cov[2], cov[2], cov[0]]),
                       (True, 3, [rect[0], rect[1], rect[1], rect[2], rect[2], rect[0]])):
        D = 0 if S == 1 else D
        G = np.stack([g for g, _ in ins]).reshape(M, rows, n, n)
        st = np.stack([_steering(S, B, ins[2 * k][1]) for k in range(M)])
        eg = api.Eig(st, wl, D, S)
        val, nul, vec, status = eg.decompose(G)
        eg.close()
        assert val.shape == (rows, M, n) and nul.shape == (rows, M, B) and vec.shape == (rows, M, n, n) and status.shape == (rows, M)
        for k in range(M):
            for j in range(rows):
                tag = "S=%d B=%d %s D=%d band %d row %d" % (S, B, "widely-linear" if wl else "linear", D, k, j)
                worst = max(worst, _check_problem(tag, G[k, j], st[k], wl, D, val[j, k], nul[j, k], vec[j, k], status[j, k]))
        if S == 1:
            assert np.abs(nul - 1.0).max() <= n * 2.0 ** -23
    print("eig S=%d B=%d: worst %.2f of the bar" % (S, B, worst))


def test_rank_deficient_matrix(api):
    """Three small-integer snapshots of S = 9 streams: G^ has rank 6 (linear) or 3 (widely linear); D = 6.  Eigenvalue,
    orthogonality and residual bars, and the trailing eigenvalues below n 2^-23 lambda_0."""
    S, B, D = 9, 9, 6
    n = 2 * S
    rng = np.random.default_rng(21)
    x = rng.integers(-3, 4, (S, 3)) + 1j * rng.integers(-3, 4, (S, 3))
    U = synth.cov_columns(x, S, 1)[0]
    G = (U @ U.T).astype(F32)                               # small integers: exact
    st = _steering(S, B, np.exp(1j * np.pi * np.arange(S) * 0.3))
    for wl, rank in ((False, 6), (True, 3)):
        eg = api.Eig(st, wl, D, S)
        val, nul, vec, status = eg.decompose(G)
        eg.close()
        _check_problem("rank-deficient %s" % ("widely-linear" if wl else "linear"), G, st, wl, D, val[0, 0], nul[0, 0], vec[0, 0],
                       status[0, 0], gap_check=False)
        assert val[0, 0, rank - 1] > 0.1 * val[0, 0, 0] * 2.0 ** -10
        assert np.abs(val[0, 0, rank:]).max() < n * 2.0 ** -23 * val[0, 0, 0]


@pytest.mark.parametrize("wl", [False, True], ids=["linear", "widely-linear"])
def test_the_scaling_is_exact_down_to_subnormal_matrices(api, wl):
    """Step 3 scales G^ by a power of two into [1, 2) whatever its size: the small-integer Gram of the rank-deficient case
    times 2^-148 -- every entry a subnormal float, exactly, and so is the linear mode's halving -- gives the same vectors and
    null spectrum bit for bit, and the eigenvalues of the integer matrix times 2^-148, rounded once more (they are
    subnormal: half a unit of 2^-148)."""
    S, B, D = 9, 9, 6
    rng = np.random.default_rng(21)
    x = rng.integers(-3, 4, (S, 3)) + 1j * rng.integers(-3, 4, (S, 3))
    U = synth.cov_columns(x, S, 1)[0]
    G = (U @ U.T).astype(F32)
    tiny = np.ldexp(G.astype(np.float64), -148).astype(F32)
    assert np.array_equal(np.ldexp(tiny.astype(np.float64), 148), G) and np.abs(tiny).max() < 2.0 ** -126
    st = _steering(S, B, np.exp(1j * np.pi * np.arange(S) * 0.3))
    eg = api.Eig(st, wl, D, S)
    val, nul, vec, status = eg.decompose(G)
    tval, tnul, tvec, tstatus = eg.decompose(tiny)
    eg.close()
    assert not status.any() and not tstatus.any()
    assert np.array_equal(_bits(tvec), _bits(vec)) and np.array_equal(_bits(tnul), _bits(nul))
    assert np.abs(np.ldexp(tval.astype(np.float64), 148) - val.astype(np.float64)).max() <= 0.5


@pytest.mark.parametrize("wl", [False, True], ids=["linear", "widely-linear"])
def test_a_diagonal_matrix_is_exact(api, wl):
    """Contract 6: G^ = diag of distinct powers of two, two of them negative, selection steering vectors: nothing is
    rotated, so the eigenvalues are the sorted diagonal, the vectors unit vectors and the null values 0 or 1, bit for bit.
    Widely linear: all 2S entries of a band distinct; linear: equal within each pair (the mode's structure)."""
    S, M, D = 9, 2, 4
    n = 2 * S
    G = np.zeros((M, 1, n, n), F32)
    d = np.zeros((M, n), F32)
    for k in range(M):
        e = (np.arange(n) * 7 + 3 * k) % n - 9              # a permutation of -9 .. 8
        d[k] = np.where(np.arange(n) % 5 == 2, -1.0, 1.0) * 2.0 ** e
        if not wl:
            d[k] = np.repeat(d[k, 0::2], 2)
        G[k, 0] = np.diag(d[k])
    st = np.zeros((M, S, S), np.complex64)
    st[:, np.arange(S), np.arange(S)] = 1.0
    eg = api.Eig(st, wl, D, S)
    val, nul, vec, status = eg.decompose(G)
    eg.close()
    assert not status.any()
    for k in range(M):
        order = np.argsort(-d[k], kind="stable")
        assert np.array_equal(_bits(val[0, k]), _bits(d[k, order]))
        want = np.zeros((n, n), F32)
        want[np.arange(n), order] = 1.0
        if not wl:
            want[1::2] = 0.0
            want[np.arange(1, n, 2), order[0::2] ^ 1] = 1.0
        assert np.array_equal(vec[0, k], want)
        sig = set(order[:D].tolist())
        assert nul[0, k].tolist() == [0.0 if (2 * s in sig or 2 * s + 1 in sig) else 1.0 for s in range(S)]


def _mixed_problem(S, B, M, rows):
    """(G (M, rows, 2S, 2S), steering (M, B, S)): cov_scene draws, each band with its own beams."""
    G = np.stack([_gram(S, "cov", 7 + i % 3)[0] if i < 3 else _gram(S, "rect", 4 + i)[0] for i in range(M * rows)]).reshape(M, rows, 2 * S, 2 * S)
    st = np.stack([np.roll(_steering(S, B, _gram(S, "cov", 7 + k)[1]), k, axis=0) for k in range(M)])
    return G, st


@pytest.mark.parametrize("wl", [False, True], ids=["linear", "widely-linear"])
def test_a_problem_depends_on_itself_alone(api, wl):
    """Contracts 2 and 3: band k, row j of an M-band, two-row call against a one-band handle decomposing that matrix
    alone, and each of nine beams against a one-beam handle."""
    S, B, M, rows, D = 9, 9, 3, 2, 4
    G, st = _mixed_problem(S, B, M, rows)
    eg = api.Eig(st, wl, D, S)
    out = eg.decompose(G)
    eg.close()
    assert not out[3].any()
    for k in range(M):
        one = api.Eig(st[k], wl, D, S)
        for j in range(rows):
            for a, b in zip(one.decompose(G[k, j]), out):
                assert np.array_equal(_bits(a[0, 0]), _bits(b[j, k])), (k, j)
        one.close()
    for b in range(B):
        one = api.Eig(st[1, b:b + 1], wl, D, 0)
        v1, n1, e1, s1 = one.decompose(G[1, 1])
        one.close()
        assert _bits(n1[0, 0, 0]) == _bits(out[1][1, 1, b]) and np.array_equal(_bits(v1[0, 0]), _bits(out[0][1, 1])), b


@pytest.mark.parametrize("wl", [False, True], ids=["linear", "widely-linear"])
def test_lower_triangle_is_never_read_and_runs_repeat(api, wl):
    """Contract 4: NaN patterns all over the strict lower triangle change no bit; contract 1: three runs, the same bits."""
    S, B, M, rows = 33, 9, 1, 2
    G, st = _mixed_problem(S, B, M, rows)
    poisoned = G.copy()
    il = np.tril_indices(2 * S, -1)
    poisoned[:, :, il[0], il[1]] = np.resize(np.frombuffer(NAN_BYTES, F32), il[0].size)
    eg = api.Eig(st, wl, 4, 5)
    first = eg.decompose(G)
    assert not first[3].any()
    for again in (eg.decompose(poisoned), eg.decompose(G), eg.decompose(G)):
        for a, b in zip(first, again):
            assert np.array_equal(_bits(a), _bits(b))
    eg.close()


def test_set_steering_and_set_signal_dim_make_a_fresh_handle(api):
    S, B, M, rows = 4, 9, 3, 1
    G, st = _mixed_problem(S, B, M, rows)
    eg = api.Eig(st[::-1], True, 2, 2)
    eg.set_steering(st)
    eg.set_signal_dim(3)
    fresh = api.Eig(st, True, 3, 2)
    for a, b in zip(eg.decompose(G), fresh.decompose(G)):
        assert np.array_equal(_bits(a), _bits(b))
    other = api.Eig(st, True, 2, 2).decompose(G)
    assert not np.array_equal(_bits(other[1]), _bits(fresh.decompose(G)[1]))          # D is not ignored
    with pytest.raises(ValueError):
        eg.set_steering(st[:, :4])
    with pytest.raises(Exception):
        eg.set_signal_dim(8)
    lin = api.Eig(st, False, 2, 2)
    with pytest.raises(Exception):
        lin.set_signal_dim(3)                               # odd in the linear mode
    for h in (eg, fresh, lin):
        h.close()


class Rows:
    """A device buffer of `rows` rows of n elements of 4 bytes, the first `shift` elements behind a guard, with at least
    MARGIN guard bytes in front of every row and behind the last (the stride is n + extra + the guard); guards and gaps
    hold the repeated `fill_bytes` pattern."""

    def __init__(self, api, rows, n, fill_bytes, extra=0, shift=0):
        self.api, self.rows, self.n = api, rows, n
        self.stride = n + extra + MARGIN // 4
        self.off = MARGIN + shift * 4
        self.nbytes = self.off + rows * self.stride * 4 + MARGIN
        self.host = np.frombuffer(np.resize(np.frombuffer(fill_bytes, np.uint8), self.nbytes).tobytes(), np.uint8).copy()
        self.d = api.DeviceArray(self.nbytes // 4)
        self.ptr = self.d.ptr + self.off

    def upload(self, a=None):
        if a is not None:
            v = self.host[self.off:self.off + self.rows * self.stride * 4].reshape(self.rows, self.stride * 4)
            v[:, :self.n * 4] = np.ascontiguousarray(a).view(np.uint8).reshape(self.rows, self.n * 4)
        self.api.check(self.d._L.sfe_dsp_memcpy_h2d(self.d.ptr, self.host.ctypes.data, self.nbytes, None))
        self.api.sync()
        return self

    def download(self):
        """(payload as (rows, 4 n) bytes, True when every byte outside the payload is what was uploaded)."""
        got = np.empty(self.nbytes, np.uint8)
        self.api.check(self.d._L.sfe_dsp_memcpy_d2h(got.ctypes.data, self.d.ptr, self.nbytes, None))
        self.api.sync()
        lo, hi = self.off, self.off + self.rows * self.stride * 4
        body, wbody = got[lo:hi].reshape(self.rows, -1), self.host[lo:hi].reshape(self.rows, -1)
        intact = (np.array_equal(got[:lo], self.host[:lo]) and np.array_equal(got[hi:], self.host[hi:])
                  and np.array_equal(body[:, self.n * 4:], wbody[:, self.n * 4:]))
        return body[:, :self.n * 4].copy(), intact

    def free(self):
        self.d.free()


@pytest.mark.parametrize("wl", [False, True], ids=["linear", "widely-linear"])
def test_any_address_and_stride_gives_the_same_bits(api, wl):
    """Contracts 2 and 8: the same matrices 1, 2 and 3 floats into larger buffers with other strides, NaN patterns all
    around every band's input rows, a sentinel all around every row of each of the four outputs."""
    S, B, E, M, rows, D = 9, 9, 4, 3, 2, 4
    n2 = 2 * S
    G, st = _mixed_problem(S, B, M, rows)
    eg = api.Eig(st, wl, D, E)
    want = eg.decompose(G)
    for shift in (1, 2, 3):
        src = Rows(api, M, rows * n2 * n2, NAN_BYTES, shift + 2, shift).upload(G)
        dV = Rows(api, rows, M * n2, SENT_BYTES, 3 - shift + 1, shift).upload()
        dN = Rows(api, rows, M * B, SENT_BYTES, shift, 4 - shift).upload()
        dE = Rows(api, rows, M * 2 * E * n2, SENT_BYTES, 7 - shift, 4 - shift).upload()
        dS = Rows(api, rows, M, SENT_BYTES, 5 - shift, 3 - shift).upload()
        try:
            assert eg.process_stream(src.ptr, rows, dV.ptr, dN.ptr, dE.ptr, dS.ptr, in_stride=src.stride, values_stride=dV.stride,
                                     null_stride=dN.stride, vectors_stride=dE.stride, status_stride=dS.stride) == rows
            api.sync()
            got = [d.download() for d in (dV, dN, dE, dS)]
            _, in_intact = src.download()
        finally:
            for d in (src, dV, dN, dE, dS):
                d.free()
        assert in_intact and all(intact for _, intact in got), shift
        for (pay, _), w in zip(got, want):
            assert np.array_equal(pay.view(np.uint32).ravel(), _bits(w).ravel()), shift
    # the optional outputs may be left out
    d_g, d_v = api.DeviceArray.from_numpy(G.ravel()), api.DeviceArray(want[0].size)
    assert eg.process_stream(d_g, rows, d_v) == rows
    assert np.array_equal(_bits(d_v.to_numpy()), _bits(want[0]).ravel())
    d_g.free()
    d_v.free()
    eg.close()


@pytest.mark.parametrize("wl", [False, True], ids=["linear", "widely-linear"])
def test_a_failed_problem_falls_back_and_leaves_its_neighbours_alone(api, wl):
    """Contract 7.  M = 3, two rows; one problem holds a NaN: status 1, NaN eigenvalues and null spectrum, the selection
    matrix; the other five match the clean run bit for bit."""
    S, B, E, M, rows = 9, 9, 4, 3, 2
    n = 2 * S
    G, st = _mixed_problem(S, B, M, rows)
    eg = api.Eig(st, wl, 4, E)
    clean = eg.decompose(G)
    bad = G.copy()
    bad[2, 0, 3, 11] = np.nan                                      # in the upper triangle: it is read
    val, nul, vec, status = eg.decompose(bad)
    eg.close()
    assert status.tolist() == [[0, 0, 1], [0, 0, 0]]
    assert np.isnan(val[0, 2]).all() and np.isnan(nul[0, 2]).all()
    assert np.array_equal(_bits(vec[0, 2]), _bits(np.eye(2 * E, n, dtype=F32)))
    vp, np_, ep, sp = api.eig_plan(st[2], bad[2, 0], wl, 4, E)
    assert sp.tolist() == [1] and np.array_equal(_bits(ep[0]), _bits(vec[0, 2])) and np.isnan(vp).all() and np.isnan(np_).all()
    for k, j in ((0, 0), (0, 1), (1, 0), (1, 1), (2, 1)):
        for a, b in zip(clean, (val, nul, vec, status)):
            assert np.array_equal(_bits(a[j, k]), _bits(b[j, k])), (k, j)


def test_the_loop_stays_on_the_device(api):
    """Cov -> Eig(E = 2).process_stream -> sfe_dsp_mvdr_load_beam -> Beam.process_stream on one stream, no host copy in
    between, linear mode.  The first eigen-beam is a complex row w with |w|^2 = 2 |v_0|^2 = 2, so its mean output power
    is 2 lambda_0(G^) and its share of the input power 2 lambda_0 / trace G^: checked against the device's own
    eigenvalues and against the float64 chain.  The bar: the eigenvalue bar of the accuracy tests, plus n 2^-23 for the
    beamformer's float32 sums, plus twice the covariance estimator's own measured error."""
    S, n, E, D = 4, N_SCENE, 2, 4
    n2 = 2 * S
    x = synth.cov_scene(S, n, 7)[0]
    cov, eg, beam = api.Cov(S, 1, n, 1.0 / n), api.Eig(None, False, D, E, n_in=S), api.Beam(np.zeros((E, S), np.complex64))
    mv = api.Mvdr(np.ones((E, S), np.complex64))           # whose load_beam hands any device matrix over
    d_x = api.DeviceArray.from_numpy(x.view(F32).ravel())
    d_g, d_val, d_vec, d_y = api.DeviceArray(n2 * n2), api.DeviceArray(n2), api.DeviceArray(2 * E * n2), api.DeviceArray(E * n * 2)
    assert cov.process_stream(d_x, n, d_g) == 1
    assert eg.process_stream(d_g, 1, d_val, None, d_vec) == 1
    mv.load_beam(beam, d_vec)
    beam.process_stream(d_x, n, d_y)
    y = d_y.to_numpy().view(np.complex64).reshape(E, n).astype(np.complex128)
    val, Gd = d_val.to_numpy().astype(np.float64), d_g.to_numpy().reshape(n2, n2)
    for d in (d_x, d_g, d_val, d_vec, d_y):
        d.free()
    for h in (cov, eg, beam, mv):
        h.close()
    U = synth.cov_columns(x, S, 1)[0]
    G64 = U @ U.T / n
    lr = synth.eig_reference(G64, None, False, D, 0)[0][0]
    l32 = np.linalg.eigh(synth.mvdr_loaded_matrix(G64.astype(F32), False, dtype=F32))[0][::-1]
    cov_err = np.linalg.norm(Gd - G64) / np.linalg.norm(G64)
    bar = max(4.0 * np.abs(l32 - lr).max() / lr[0], n2 * 2.0 ** -23) + n2 * 2.0 ** -23 + 2.0 * cov_err
    share_out = (np.abs(y[0]) ** 2).sum() / (np.abs(x.astype(np.complex128)) ** 2).sum()
    share_dev, share_ref = 2.0 * val[0] / val.sum(), 2.0 * lr[0] / lr.sum()
    print("cov -> eig -> load_beam -> beam: share of eigen-beam 0: output %.8f, device eigenvalues %.8f, float64 %.8f, bar %.1e"
          % (share_out, share_dev, share_ref, bar))
    assert share_ref > 0.9
    assert abs(share_out - share_dev) <= bar * share_ref and abs(share_out - share_ref) <= bar * share_ref


def test_refusals_launch_nothing(api, L, hip):
    S, B, E, M, rows = 3, 2, 2, 2, 2
    n2 = 2 * S
    gram, mat = n2 * n2, 2 * E * n2
    G, st = _mixed_problem(S, B, M, rows)
    eg = api.Eig(st, False, 2, E)
    d_g = api.DeviceArray.from_numpy(np.concatenate([G.ravel(), np.zeros(64, F32)]))
    sentinel = np.full(rows * M * mat + 64, SENT, F32)
    d_v, d_n, d_e, d_s = (api.DeviceArray.from_numpy(sentinel) for _ in range(4))
    lib = L.load()
    k = C.c_size_t(7)
    is_, vs, ns, es, ss = rows * gram, M * n2, M * B, M * mat, M

    def call(pg=d_g.ptr, n_rows=rows, in_stride=is_, pv=d_v.ptr, vstride=vs, pn=d_n.ptr, nstride=ns, pe=d_e.ptr, estride=es,
             pst=d_s.ptr, sstride=ss, stream=None, h=None):
        return lib.sfe_dsp_eig_process_stream(h or eg._h, pg, n_rows, in_stride, pv, vstride, pn, nstride, pe, estride, pst, sstride,
                                              C.byref(k), stream)

    assert call(vstride=vs - 1) == L.SFE_ERANGE                      # a row's block one float short, each of the four
    assert call(nstride=ns - 1) == L.SFE_ERANGE
    assert call(estride=es - 1) == L.SFE_ERANGE
    assert call(sstride=ss - 1) == L.SFE_ERANGE
    assert call(in_stride=is_ - 1) == L.SFE_EINVAL                   # in_stride below n_rows (2S)^2
    assert call(pg=None) == L.SFE_EINVAL                             # null input
    assert call(pv=None) == L.SFE_EINVAL                             # null eigenvalue output
    assert call(pg=d_g.ptr + 2) == L.SFE_EINVAL                      # misaligned, each of the five
    assert call(pv=d_v.ptr + 1) == L.SFE_EINVAL
    assert call(pn=d_n.ptr + 2) == L.SFE_EINVAL
    assert call(pe=d_e.ptr + 3) == L.SFE_EINVAL
    assert call(pst=d_s.ptr + 3) == L.SFE_EINVAL
    assert call(pv=d_g.ptr + 4 * gram) == L.SFE_EINVAL               # each output over the input
    assert call(pn=d_g.ptr + 4 * (M * is_ - 1)) == L.SFE_EINVAL
    assert call(pe=d_g.ptr + 4 * 8) == L.SFE_EINVAL
    assert call(pst=d_g.ptr) == L.SFE_EINVAL
    big = (1 << 31) // gram
    assert call(n_rows=big, in_stride=big * gram) == L.SFE_EINVAL    # 2^31 / (2S)^2 rows
    assert lib.sfe_dsp_eig_process_stream(eg._h, d_g.ptr, rows, is_, d_v.ptr, vs, None, 0, None, 0, None, 0, None, None) == L.SFE_EINVAL   # no counter
    assert k.value == 0
    assert call(n_rows=0, in_stride=0) == L.SFE_OK and k.value == 0  # no rows: a no-op
    # a capturing stream: the call is refused, and the capture ends as an empty graph
    s = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(s)) == 0
    assert hip.hipStreamBeginCapture(s, 2) == 0            # relaxed mode: the refused call launches nothing
    try:
        rc = call(stream=s.value)
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
    # a live handle of another block is refused by every eig function, and eig's destroy frees nothing of it
    other = api.Mvdr(st, False, 1e-3)
    fp = C.POINTER(C.c_float)
    assert call(h=other._h) == L.SFE_EINVAL and k.value == 0
    assert lib.sfe_dsp_eig_set_steering(other._h, st.view(F32).ctypes.data_as(fp)) == L.SFE_EINVAL
    assert lib.sfe_dsp_eig_set_signal_dim(other._h, 2) == L.SFE_EINVAL
    assert lib.sfe_dsp_eig_destroy(other._h) == L.SFE_OK
    assert not other.solve(G)[2].any()                                              # still alive
    other.close()
    assert lib.sfe_dsp_eig_set_steering(eg._h, None) == L.SFE_EINVAL
    assert lib.sfe_dsp_eig_set_signal_dim(eg._h, 3) == L.SFE_EINVAL and lib.sfe_dsp_last_error().startswith(b"eig: ")
    nobeams = api.Eig(None, False, 2, E, n_in=S, n_bands=M)
    assert lib.sfe_dsp_eig_set_steering(nobeams._h, st.view(F32).ctypes.data_as(fp)) == L.SFE_EINVAL
    api.sync()
    for d in (d_v, d_n, d_e, d_s):
        assert np.array_equal(_bits(d.to_numpy()), _bits(sentinel))
    assert np.array_equal(_bits(d_g.to_numpy(G.size)), _bits(G).ravel())
    # the next good call is a fresh handle's; a handle of no beams ignores d_null and writes the same eigenvalues
    assert call() == L.SFE_OK and k.value == rows
    want = api.Eig(st, False, 2, E).decompose(G)
    assert np.array_equal(_bits(d_v.to_numpy(rows * vs)), _bits(want[0]).ravel())
    assert np.array_equal(_bits(d_n.to_numpy(rows * ns)), _bits(want[1]).ravel())
    assert np.array_equal(_bits(d_e.to_numpy(rows * es)), _bits(want[2]).ravel())
    assert np.array_equal(d_s.to_numpy(rows * ss).view(np.int32), want[3].ravel())
    assert np.array_equal(_bits(d_e.to_numpy()[rows * es:]), _bits(sentinel[rows * es:]))
    got = nobeams.decompose(G)
    assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(_bits(got[2]), _bits(want[2])) and got[1].shape == (rows, M, 0)
    nobeams.close()
    eg.close()
    for d in (d_g, d_v, d_n, d_e, d_s):
        d.free()
