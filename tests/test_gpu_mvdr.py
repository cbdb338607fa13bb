"""The adaptive beamforming weight solver on the GPU (sfe_dsp_mvdr_*, csrc/mvdr.hip) against the float64 statement of its
law (synth.mvdr_reference), the parts of the contract that are about bits, the hand-over to a live beamformer
(sfe_dsp_mvdr_load_beam), the device-resident loop cov -> mvdr -> load_beam -> beam, and the refusals.

The accuracy bar is measured, not fixed.  For every input the test also evaluates the law in float32 through LAPACK
(scipy.linalg.cho_factor / cho_solve on float32 arrays, the rest in float32 numpy) and allows

    max(4 x that error, n 2^-23)            n = 2S

-- 4 for another elimination and summation order without pivoting, the floor a few roundings per output of an n-term dot
product.  The errors are, per problem, the relative Frobenius error of R and the relative error of each power against the
float64 reference on the same float32 G; "that error" of the powers is LAPACK's largest over the problem's beams (one
power is one number: the ratio of two single roundings says nothing, so the accuracy cases carry at least eight beams;
B = 1 is covered bit for bit against them by the one-beam contract).  What keeps the bar honest: every input used has
cond_2(G^) <= 1e6 in float64, asserted, so float32 can factor it.  The rectilinear scene at S = 64, load_rel = 1e-4 has
cond 1.2e6 and is left out for that reason alone.

Shapes are the smallest at which the kernel can go wrong: S = 1 (n = 2, the closed form of the widely-linear mode and
less than one lane group), 8 (n = 16: two lanes' worth per slot), 9 (n = 18: ragged against the eight lanes of a slot),
33, 64 (the LDS maximum); B = 1, 8 (one wave's slots in the linear mode), 9, 64 (four passes in the widely-linear mode);
M = 1, 3; one and two rows."""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg

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
        G = synth.cov_reference(x, S, 1, N_SCENE, 1.0 / N_SCENE)[0, 0].astype(F32)
        G.setflags(write=False)
        _grams[key] = (G, a)
    return _grams[key]


def _steering(S, B, a_d):
    """(B, S) complex64: the scene's desired steering vector, then a sine grid of scan directions."""
    u = -1.0 + (2.0 * np.arange(B) + 1.0) / B
    st = np.exp(1j * np.pi * u[:, None] * np.arange(S)[None, :])
    st[0] = a_d
    return st.astype(np.complex64)


def _lapack32(G, steering, wl, load_rel):
    """The law in float32: LAPACK's Cholesky and substitutions, the rest in float32 numpy.  (R (2B, 2S), power (B,))."""
    Gh = synth.mvdr_loaded_matrix(G, wl, load_rel, 0.0, dtype=F32)
    c = scipy.linalg.cho_factor(Gh, lower=True)
    B, n = steering.shape[0], G.shape[0]
    R, pw = np.empty((2 * B, n), F32), np.empty(B, F32)
    for b in range(B):
        A2 = synth.mvdr_rhs(steering[b], dtype=F32)
        Z = scipy.linalg.cho_solve(c, A2).astype(F32)
        if wl:
            Q = (A2.T @ Z).astype(F32)
            q00, q01, q11 = Q[0, 0], Q[0, 1], Q[1, 1]
            det = F32(q00 * q11 - q01 * q01)
            R[2 * b], R[2 * b + 1] = (q11 * Z[:, 0] - q01 * Z[:, 1]) / det, (q00 * Z[:, 1] - q01 * Z[:, 0]) / det
            pw[b] = (q00 + q11) / det
        else:
            q = F32(A2[:, 0] @ Z[:, 0])
            r = Z[:, 0] / q
            R[2 * b], R[2 * b + 1, 0::2], R[2 * b + 1, 1::2] = r, -r[1::2], r[0::2]
            pw[b] = F32(2.0) / q
    return R, pw


def _errors(R, pw, Rr, pr):
    return np.linalg.norm(R.astype(np.float64) - Rr) / np.linalg.norm(Rr), np.abs(pw.astype(np.float64) - pr) / pr


def _check_problem(tag, G, steering, wl, load_rel, R, pw, status):
    """One problem against the bar of the module's docstring; returns the worst ratio to the bar."""
    n = G.shape[0]
    cond = np.linalg.cond(synth.mvdr_loaded_matrix(G, wl, load_rel, 0.0))
    assert cond <= 1e6, (tag, cond)
    Rr, pr, sr = synth.mvdr_reference(G, steering, wl, load_rel, 0.0)
    assert sr[0] == 0 and status == 0, (tag, status)
    assert np.isfinite(R).all() and np.isfinite(pw).all(), tag
    eR, eP = _errors(R, pw, Rr[0], pr[0])
    lR, lP = _errors(*_lapack32(G, steering, wl, load_rel), Rr[0], pr[0])
    floor = n * 2.0 ** -23
    barR, barP = max(4.0 * lR, floor), max(4.0 * lP.max(), floor)
    ratio = max(eR / barR, eP.max() / barP)
    print("mvdr %s cond %.2g: R %.2e (LAPACK %.2e), power %.2e (LAPACK %.2e): %.2f of the bar" % (tag, cond, eR, lR, eP.max(), lP.max(), ratio))
    assert eR <= barR and (eP <= barP).all(), (tag, eR, barR, eP.max(), barP)
    if not wl:          # contract 4: the exact W-only structure
        assert np.array_equal(_bits(R[1::2, 0::2]), _bits(-R[0::2, 1::2])) and np.array_equal(_bits(R[1::2, 1::2]), _bits(R[0::2, 0::2])), tag
    return ratio


ACC_B = {1: 9, 8: 8, 9: 64, 33: 9, 64: 64}


@pytest.mark.parametrize("S", sorted(ACC_B))
def test_accuracy_against_float64(api, S):
    """M = 3 bands of two rows each: six problems per call.  Linear mode: cov_scene draws 7 .. 12.  Widely-linear mode:
    cov_scene draws 7 .. 9 and the rectilinear scene's draws 7 .. 9."""
    B, M, rows = ACC_B[S], 3, 2
    worst = 0.0
    for wl in (False, True):
        for load_rel in (1e-4, 1e-2):
            rect = wl and not (S == 64 and load_rel == 1e-4)        # cond 1.2e6 there: see the module's docstring
            ins = [_gram(S, "cov", 7 + i) for i in range(3)] + [_gram(S, "rect" if rect else "cov", (7 if rect else 10) + i) for i in range(3)]
            G = np.stack([g for g, _ in ins]).reshape(M, rows, 2 * S, 2 * S)
            st = np.stack([_steering(S, B, ins[2 * k][1]) for k in range(M)])
            mv = api.Mvdr(st, wl, load_rel)
            R, pw, status = mv.solve(G)
            mv.close()
            assert R.shape == (rows, M, 2 * B, 2 * S) and pw.shape == (rows, M, B) and status.shape == (rows, M)
            for k in range(M):
                for j in range(rows):
                    tag = "S=%d B=%d %s load_rel=%g band %d row %d" % (S, B, "widely-linear" if wl else "linear", load_rel, k, j)
                    worst = max(worst, _check_problem(tag, G[k, j], st[k], wl, load_rel, R[j, k], pw[j, k], status[j, k]))
    print("mvdr S=%d B=%d: worst %.2f of the bar" % (S, B, worst))


@pytest.mark.parametrize("wl", [False, True], ids=["linear", "widely-linear"])
def test_selection_is_exact(api, wl):
    """G = diag of even powers of two, zero loading, unit steering vectors: every square root, quotient and product is
    exact, so R must be the selection matrix and the power the sum of the chosen pair's diagonal entries, bit for bit.
    Widely linear: all entries of a band distinct within each pair; linear: equal within each pair."""
    S, B, M = 9, 9, 2
    exps = np.array([-4, -2, 0, 2, 4])
    G = np.zeros((M, 1, 2 * S, 2 * S), F32)
    for k in range(M):
        for s in range(S):
            e0, e1 = exps[(s + k) % 5], exps[(s + k + 1 + s // 5) % 5]
            G[k, 0, 2 * s, 2 * s], G[k, 0, 2 * s + 1, 2 * s + 1] = 2.0 ** e0, 2.0 ** (e1 if wl else e0)
    pick = np.array([[3, 0, 7, 8, 1, 5, 2, 6, 4], [8, 6, 0, 1, 7, 2, 4, 3, 5]])       # s_b of band k: no symmetry to hide a transpose
    st = np.zeros((M, B, S), np.complex64)
    for k in range(M):
        st[k, np.arange(B), pick[k]] = 1.0
    mv = api.Mvdr(st, wl, 0.0, 0.0)
    R, pw, status = mv.solve(G)
    mv.close()
    want = np.zeros((M, 2 * B, 2 * S), F32)
    for k in range(M):
        want[k, 2 * np.arange(B), 2 * pick[k]] = 1.0
        want[k, 2 * np.arange(B) + 1, 2 * pick[k] + 1] = 1.0
    assert not status.any()
    assert np.array_equal(R[0], want)
    d = np.diagonal(G[:, 0], axis1=1, axis2=2)
    assert np.array_equal(pw[0], np.stack([d[k, 2 * pick[k]] + d[k, 2 * pick[k] + 1] for k in range(M)]))


def _mixed_problem(S, B, M, rows):
    """(G (M, rows, 2S, 2S), steering (M, B, S)): cov_scene draws, each band with its own beams."""
    G = np.stack([_gram(S, "cov", 7 + i)[0] for i in range(M * rows)]).reshape(M, rows, 2 * S, 2 * S)
    st = np.stack([np.roll(_steering(S, B, _gram(S, "cov", 7 + rows * k)[1]), k, axis=0) for k in range(M)])
    return G, st


@pytest.mark.parametrize("wl", [False, True], ids=["linear", "widely-linear"])
def test_a_problem_depends_on_itself_alone(api, wl):
    """Contracts 2 and 3: band k, row j of an M-band, two-row call against a one-band handle solving that matrix alone,
    and each beam against a one-beam handle; B = 9."""
    S, B, M, rows = 9, 9, 3, 2
    G, st = _mixed_problem(S, B, M, rows)
    mv = api.Mvdr(st, wl, 1e-3)
    R, pw, status = mv.solve(G)
    mv.close()
    assert not status.any()
    for k in range(M):
        one = api.Mvdr(st[k], wl, 1e-3)
        for j in range(rows):
            r1, p1, s1 = one.solve(G[k, j])
            assert np.array_equal(_bits(r1[0, 0]), _bits(R[j, k])) and np.array_equal(_bits(p1[0, 0]), _bits(pw[j, k])), (k, j)
        one.close()
    for b in range(B):
        one = api.Mvdr(st[1, b:b + 1], wl, 1e-3)
        r1, p1, s1 = one.solve(G[1, 1])
        one.close()
        assert np.array_equal(_bits(r1[0, 0]), _bits(R[1, 1, 2 * b:2 * b + 2])) and _bits(p1[0, 0, 0]) == _bits(pw[1, 1, b]), b


@pytest.mark.parametrize("wl", [False, True], ids=["linear", "widely-linear"])
def test_lower_triangle_is_never_read_and_runs_repeat(api, wl):
    """Contract 5: NaN patterns all over the strict lower triangle change no bit; contract 1: three runs, the same bits."""
    S, B, M, rows = 33, 8, 1, 2
    G, st = _mixed_problem(S, B, M, rows)
    poisoned = G.copy()
    il = np.tril_indices(2 * S, -1)
    poisoned[:, :, il[0], il[1]] = np.resize(np.frombuffer(NAN_BYTES, F32), il[0].size)
    mv = api.Mvdr(st, wl, 1e-3)
    first = mv.solve(G)
    assert not first[2].any()
    for again in (mv.solve(poisoned), mv.solve(G), mv.solve(G)):
        for a, b in zip(first, again):
            assert np.array_equal(_bits(a), _bits(b))
    mv.close()


def test_set_steering_and_set_loading_make_a_fresh_handle(api):
    S, B, M, rows = 8, 8, 3, 1
    G, st = _mixed_problem(S, B, M, rows)
    mv = api.Mvdr(st[::-1], True, 1e-2, 1e-9)
    mv.set_steering(st)
    mv.set_loading(1e-4, 0.0)
    fresh = api.Mvdr(st, True, 1e-4, 0.0)
    for a, b in zip(mv.solve(G), fresh.solve(G)):
        assert np.array_equal(_bits(a), _bits(b))
    with pytest.raises(ValueError):
        mv.set_steering(st[:, :4])
    with pytest.raises(Exception):
        mv.set_loading(-1.0)
    mv.close()
    fresh.close()


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
    """Contracts 2 and 7: the same matrices 1, 2 and 3 floats into larger buffers with other strides, NaN patterns all
    around every band's input rows, a sentinel all around every row of each of the three outputs."""
    S, B, M, rows = 9, 9, 3, 2
    n2 = 2 * S
    G, st = _mixed_problem(S, B, M, rows)
    mv = api.Mvdr(st, wl, 1e-3)
    R, pw, status = mv.solve(G)
    for shift in (1, 2, 3):
        src = Rows(api, M, rows * n2 * n2, NAN_BYTES, shift + 2, shift).upload(G)
        dR = Rows(api, rows, M * 2 * B * n2, SENT_BYTES, 7 - shift, 4 - shift).upload()
        dP = Rows(api, rows, M * B, SENT_BYTES, shift, shift).upload()
        dS = Rows(api, rows, M, SENT_BYTES, 5 - shift, 3 - shift).upload()
        try:
            assert mv.process_stream(src.ptr, rows, dR.ptr, dP.ptr, dS.ptr, in_stride=src.stride, out_stride=dR.stride,
                                     power_stride=dP.stride, status_stride=dS.stride) == rows
            api.sync()
            got = [d.download() for d in (dR, dP, dS)]
            _, in_intact = src.download()
        finally:
            for d in (src, dR, dP, dS):
                d.free()
        assert in_intact and all(intact for _, intact in got), shift
        for (pay, _), want in zip(got, (R, pw, status)):
            assert np.array_equal(pay.view(np.uint32).ravel(), _bits(want).ravel()), shift
    # the optional outputs may be left out
    d_g, d_R = api.DeviceArray.from_numpy(G.ravel()), api.DeviceArray(R.size)
    assert mv.process_stream(d_g, rows, d_R) == rows
    assert np.array_equal(_bits(d_R.to_numpy()), _bits(R).ravel())
    d_g.free()
    d_R.free()
    mv.close()


@pytest.mark.parametrize("wl", [False, True], ids=["linear", "widely-linear"])
def test_failed_problems_fall_back_and_leave_their_neighbours_alone(api, wl):
    """Contract 6.  M = 3, two rows; one problem is -I, one holds a NaN: status 1, the host plan's fallback bits, NaN
    powers; the other four match the clean run bit for bit."""
    S, B, M, rows = 9, 8, 3, 2
    G, st = _mixed_problem(S, B, M, rows)
    mv = api.Mvdr(st, wl, 1e-3)
    clean = mv.solve(G)
    bad = G.copy()
    bad[0, 1] = -np.eye(2 * S, dtype=F32)
    bad[2, 0, 3, 11] = np.nan                                      # in the upper triangle: it is read
    R, pw, status = mv.solve(bad)
    mv.close()
    assert status.tolist() == [[0, 0, 1], [1, 0, 0]]
    for k, j in ((0, 1), (2, 0)):
        Rp, pp, sp = api.mvdr_plan(st[k], bad[k, j], wl, 1e-3)
        assert sp.tolist() == [1] and np.isnan(pp).all()
        assert np.array_equal(_bits(R[j, k]), _bits(Rp[0])) and np.isnan(pw[j, k]).all()
        assert np.abs(R[j, k] - synth.mvdr_fallback(st[k])[0]).max() <= 2.0 ** -24 * np.abs(R[j, k]).max()
    for k, j in ((0, 0), (1, 0), (1, 1), (2, 1)):
        for a, b in zip(clean, (R, pw, status)):
            assert np.array_equal(_bits(a[j, k]), _bits(b[j, k])), (k, j)


def test_a_failed_beam_falls_back_alone(api):
    """Status 2.  G = 2e-38 I factors, but z = u / 2e-38 and q = |a|^2 / 2e-38: with |a|^2 = 16 q overflows and that beam
    fails, with |a|^2 = 1 the linear mode's q = 5e37 is fine (the widely-linear det Q = q^2 overflows for both)."""
    S = 4
    st = np.stack([np.full(S, 0.5), np.full(S, 2.0)]).astype(np.complex64)
    G = (F32(2e-38) * np.eye(2 * S, dtype=F32))
    fb = api.mvdr_plan(st, -np.eye(2 * S, dtype=F32))[0][0]          # the fallback bits, from the host plan
    mv = api.Mvdr(st, False)
    R, pw, status = mv.solve(G)
    mv.close()
    assert status.tolist() == [[2]]
    assert np.array_equal(_bits(R[0, 0, 2:]), _bits(fb[2:])) and np.isnan(pw[0, 0, 1])
    assert np.array_equal(R[0, 0, :2], fb[:2]) and np.isfinite(pw[0, 0, 0])       # a good beam: u / |a|^2, exact here
    assert abs(float(pw[0, 0, 0]) / 4e-38 - 1.0) < 1e-6                          # 2 / q, q = |a|^2 / 2e-38
    mw = api.Mvdr(st, True)
    R, pw, status = mw.solve(G)
    mw.close()
    assert status.tolist() == [[2]] and np.array_equal(_bits(R[0, 0]), _bits(fb)) and np.isnan(pw).all()


@pytest.mark.parametrize("shape", [(9, 9, 3), (64, 64, 1)], ids=["S9-B9-M3", "S64-B64-M1"])
def test_load_beam_is_set_weights_from_the_device(api, shape):
    """A Beam created from zeros and handed sfe_dsp_beam_plan's real matrix of random (W, V) from a device buffer gives
    the bits of a Beam created from (W, V); a call enqueued before the hand-over on the same stream keeps the old
    weights."""
    S, B, M = shape
    n = 200
    rng = np.random.default_rng(17)
    W = (rng.standard_normal((M, B, S)) + 1j * rng.standard_normal((M, B, S))).astype(np.complex64) / S
    V = (rng.standard_normal((M, B, S)) + 1j * rng.standard_normal((M, B, S))).astype(np.complex64) / S
    x = np.stack([synth.synth_cf32(M * n, ch=s).view(np.complex64).reshape(M, n) for s in range(S)])
    ref, late = api.Beam(W, V), api.Beam(np.zeros_like(W))
    want = ref.mix(x)
    assert np.abs(want).max() > 1e-3
    mv = api.Mvdr(np.ones((M, B, S), np.complex64))
    d_R = api.DeviceArray.from_numpy(api.beam_plan(W, V).ravel())
    d_x = api.DeviceArray.from_numpy(x.view(F32).ravel())
    d_before, d_after = api.DeviceArray(B * M * n * 2), api.DeviceArray(B * M * n * 2)
    late.process_stream(d_x, n, d_before)                   # enqueued first: the zero weights
    mv.load_beam(late, d_R)
    late.process_stream(d_x, n, d_after)
    before = d_before.to_numpy().view(np.complex64).reshape(B, M, n)
    after = d_after.to_numpy().view(np.complex64).reshape(B, M, n)
    assert not before.any()
    assert np.array_equal(_bits(after.view(F32)), _bits(want.view(F32)))
    # and set_weights afterwards still replaces what was loaded
    late.set_weights(V, W)
    assert np.array_equal(_bits(late.mix(x).view(F32)), _bits(api.Beam(V, W).mix(x).view(F32)))
    for d in (d_R, d_x, d_before, d_after):
        d.free()
    for h in (ref, late, mv):
        h.close()


def _sir_db(y_d, y_i):
    return 10.0 * np.log10((np.abs(y_d.astype(np.complex128)) ** 2).sum() / (np.abs(y_i.astype(np.complex128)) ** 2).sum())


def test_the_loop_stays_on_the_device(api):
    """Cov -> Mvdr.process_stream -> load_beam -> Beam.process_stream on one stream, no host copy in between, on a scene
    with an interferer 30 dB above the signal.  One wrong entry costs tens of dB; the 1 dB is not a measurement of the
    kernel."""
    S, n, load_rel = 4, N_SCENE, 1e-4
    x, x_d, x_i, a = synth.cov_scene(S, n, 7)
    C64, _ = synth.cov_from_gram(synth.cov_reference(x, S, 1, n, 1.0 / n)[0, 0])
    w64 = synth.mvdr_weights(C64, a, load_rel)[0, 0].astype(np.complex128)
    sir_ref = _sir_db(w64 @ x_d.astype(np.complex128), w64 @ x_i.astype(np.complex128))
    cov, mv, beam = api.Cov(S, 1, n, 1.0 / n), api.Mvdr(a[None, :], False, load_rel), api.Beam(np.zeros((1, S), np.complex64))
    d_x, d_parts = api.DeviceArray.from_numpy(x.view(F32).ravel()), api.DeviceArray.from_numpy(np.stack([x_d, x_i]).view(F32).ravel())
    d_g, d_R, d_y = api.DeviceArray(4 * S * S), api.DeviceArray(4 * S), api.DeviceArray(2 * n * 2)
    assert cov.process_stream(d_x, n, d_g) == 1
    assert mv.process_stream(d_g, 1, d_R) == 1
    mv.load_beam(beam, d_R)
    beam.process_stream(d_parts.ptr, n, d_y.ptr)                        # the desired part alone,
    beam.process_stream(d_parts.ptr + 8 * S * n, n, d_y.ptr + 8 * n)    # then the interferer's
    y = d_y.to_numpy().view(np.complex64).reshape(2, n)
    sir_gpu = _sir_db(y[0], y[1])
    for d in (d_x, d_parts, d_g, d_R, d_y):
        d.free()
    print("cov -> mvdr -> load_beam -> beam: float64 chain %.2f dB, device chain %.2f dB" % (sir_ref, sir_gpu))
    assert sir_ref >= 40.0
    assert abs(sir_gpu - sir_ref) <= 1.0


def test_the_mode_flag_is_not_ignored(api):
    """A rectilinear interferer and two elements: the widely-linear solver has a degree of freedom the linear one lacks.
    The float64 references differ by >= 3 dB; the GPU matches each within the accuracy bar (eight beams: the desired
    direction and seven scan directions)."""
    S, B, load_rel = 2, 8, 1e-2
    x, x_d, x_i, a = synth.mvdr_scene_rectilinear(S, N_SCENE, 7)
    G = _gram(S, "rect", 7)[0]
    st = _steering(S, B, a)
    sir = {}
    for wl in (False, True):
        Rr = synth.mvdr_reference(G, st, wl, load_rel)[0][0, :2]
        y = [Rr @ synth.cov_columns(p, S, 1)[0] for p in (x_d, x_i)]
        sir[wl] = 10.0 * np.log10((y[0] ** 2).sum() / (y[1] ** 2).sum())
        mv = api.Mvdr(st, wl, load_rel)
        R, pw, status = mv.solve(G)
        mv.close()
        _check_problem("rectilinear S=2 %s" % ("widely-linear" if wl else "linear"), G, st, wl, load_rel, R[0, 0], pw[0, 0], status[0, 0])
    print("rectilinear scene, S = 2: linear %.1f dB, widely linear %.1f dB" % (sir[False], sir[True]))
    assert sir[True] >= sir[False] + 3.0


def test_refusals_launch_nothing(api, L, hip):
    S, B, M, rows = 3, 2, 2, 2
    n2 = 2 * S
    gram, mat = n2 * n2, 2 * B * n2
    G, st = _mixed_problem(S, B, M, rows)
    mv = api.Mvdr(st, False, 1e-3)
    d_g = api.DeviceArray.from_numpy(np.concatenate([G.ravel(), np.zeros(64, F32)]))
    sentinel = np.full(rows * M * mat + 64, SENT, F32)
    d_R, d_p, d_s = (api.DeviceArray.from_numpy(sentinel) for _ in range(3))
    lib = L.load()
    k = C.c_size_t(7)
    is_, os_, ps, ss = rows * gram, M * mat, M * B, M

    def call(pg, n_rows, in_stride, pR, out_stride, pp=d_p.ptr, pstride=ps, pst=d_s.ptr, sstride=ss, stream=None, h=None):
        return lib.sfe_dsp_mvdr_process_stream(h or mv._h, pg, n_rows, in_stride, pR, out_stride, pp, pstride, pst, sstride, C.byref(k), stream)

    assert call(d_g.ptr, rows, is_, d_R.ptr, os_ - 1) == L.SFE_ERANGE               # a row's block one float short
    assert call(d_g.ptr, rows, is_, d_R.ptr, os_, pstride=ps - 1) == L.SFE_ERANGE
    assert call(d_g.ptr, rows, is_, d_R.ptr, os_, sstride=ss - 1) == L.SFE_ERANGE
    assert call(d_g.ptr, rows, is_ - 1, d_R.ptr, os_) == L.SFE_EINVAL               # in_stride below n_rows (2S)^2
    assert call(None, rows, is_, d_R.ptr, os_) == L.SFE_EINVAL                      # null input
    assert call(d_g.ptr, rows, is_, None, os_) == L.SFE_EINVAL                      # null matrix output
    assert call(d_g.ptr + 2, rows, is_, d_R.ptr, os_) == L.SFE_EINVAL               # misaligned, each of the four
    assert call(d_g.ptr, rows, is_, d_R.ptr + 1, os_) == L.SFE_EINVAL
    assert call(d_g.ptr, rows, is_, d_R.ptr, os_, pp=d_p.ptr + 2) == L.SFE_EINVAL
    assert call(d_g.ptr, rows, is_, d_R.ptr, os_, pst=d_s.ptr + 3) == L.SFE_EINVAL
    assert call(d_g.ptr, rows, is_, d_g.ptr + 4 * gram, os_) == L.SFE_EINVAL        # each output over the input
    assert call(d_g.ptr, rows, is_, d_R.ptr, os_, pp=d_g.ptr + 4 * (M * is_ - 1)) == L.SFE_EINVAL
    assert call(d_g.ptr, rows, is_, d_R.ptr, os_, pst=d_g.ptr) == L.SFE_EINVAL
    big = (1 << 31) // gram
    assert call(d_g.ptr, big, big * gram, d_R.ptr, os_) == L.SFE_EINVAL             # 2^31 / (2S)^2 rows
    assert lib.sfe_dsp_mvdr_process_stream(mv._h, d_g.ptr, rows, is_, d_R.ptr, os_, None, 0, None, 0, None, None) == L.SFE_EINVAL      # no counter
    assert k.value == 0
    assert call(d_g.ptr, 0, 0, d_R.ptr, 0) == L.SFE_OK and k.value == 0             # no rows: a no-op
    # the hand-over: a non-beam handle, a null handle, a null and a misaligned matrix
    beam = api.Beam(np.ones((M, B, S), np.complex64))
    x = np.stack([synth.synth_cf32(M * 64, ch=s).view(np.complex64).reshape(M, 64) for s in range(S)])
    y0 = beam.mix(x)
    assert lib.sfe_dsp_mvdr_load_beam(mv._h, d_R.ptr, None) == L.SFE_EINVAL and b"beamformer" in lib.sfe_dsp_last_error()
    assert lib.sfe_dsp_mvdr_load_beam(None, d_R.ptr, None) == L.SFE_EINVAL
    assert lib.sfe_dsp_mvdr_load_beam(beam._h, None, None) == L.SFE_EINVAL
    assert lib.sfe_dsp_mvdr_load_beam(beam._h, d_R.ptr + 2, None) == L.SFE_EINVAL
    # a capturing stream: both calls refused, and the capture ends as an empty graph
    s = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(s)) == 0
    assert hip.hipStreamBeginCapture(s, 2) == 0            # relaxed mode: the refused calls launch nothing
    try:
        rc = call(d_g.ptr, rows, is_, d_R.ptr, os_, stream=s.value)
        msg = lib.sfe_dsp_last_error()
        rc2 = lib.sfe_dsp_mvdr_load_beam(beam._h, d_R.ptr, s.value)
        msg2 = lib.sfe_dsp_last_error()
    finally:
        g = C.c_void_p()
        ended = hip.hipStreamEndCapture(s, C.byref(g))
    nodes = C.c_size_t(0)
    if g.value:
        assert hip.hipGraphGetNodes(g, None, C.byref(nodes)) == 0
        hip.hipGraphDestroy(g)
    hip.hipStreamDestroy(s)
    assert rc == L.SFE_ESTATE and k.value == 0 and b"graph capture is not supported" in msg
    assert rc2 == L.SFE_ESTATE and b"graph capture is not supported" in msg2
    assert ended == 0 and (not g.value or nodes.value == 0)
    # a live handle of another block is refused by every mvdr function, and mvdr's destroy frees nothing of it
    other = api.Iir(synth.iir_dc_blocker(0.995))
    fp = C.POINTER(C.c_float)
    assert call(d_g.ptr, rows, is_, d_R.ptr, os_, h=other._h) == L.SFE_EINVAL and k.value == 0
    assert lib.sfe_dsp_mvdr_set_steering(other._h, st.view(F32).ctypes.data_as(fp)) == L.SFE_EINVAL
    assert lib.sfe_dsp_mvdr_set_loading(other._h, 0.0, 0.0) == L.SFE_EINVAL
    assert lib.sfe_dsp_mvdr_load_beam(other._h, d_R.ptr, None) == L.SFE_EINVAL
    assert lib.sfe_dsp_mvdr_destroy(other._h) == L.SFE_OK
    assert np.isfinite(other.filter(x[0, 0, :other.block])).all()                   # still alive
    assert lib.sfe_dsp_mvdr_set_steering(mv._h, None) == L.SFE_EINVAL
    api.sync()
    for d in (d_R, d_p, d_s):
        assert np.array_equal(_bits(d.to_numpy()), _bits(sentinel))
    assert np.array_equal(_bits(d_g.to_numpy(G.size)), _bits(G).ravel())
    assert np.array_equal(_bits(beam.mix(x).view(F32)), _bits(y0.view(F32)))        # no refused hand-over touched the weights
    # the next good call is a fresh handle's
    assert call(d_g.ptr, rows, is_, d_R.ptr, os_) == L.SFE_OK and k.value == rows
    want = api.Mvdr(st, False, 1e-3).solve(G)
    assert np.array_equal(_bits(d_R.to_numpy(rows * os_)), _bits(want[0]).ravel())
    assert np.array_equal(_bits(d_p.to_numpy(rows * ps)), _bits(want[1]).ravel())
    assert np.array_equal(d_s.to_numpy(rows * ss).view(np.int32), want[2].ravel())
    assert np.array_equal(_bits(d_R.to_numpy()[rows * os_:]), _bits(sentinel[rows * os_:]))
    for d in (d_g, d_R, d_p, d_s):
        d.free()
