"""The eigen-decomposition / MUSIC direction finder (sfe_dsp_eig_*) without a GPU: the C ABI's declarations and exports,
the host-only planner -- its refusals, its float64 Jacobi against the independent numpy statement of the law
(synth.eig_reference, numpy.linalg.eigh), its failure path, the exact diagonal case -- the no-GPU refusal, the MUSIC
answer on the project's two scenes, the build lists and the kernel's register budget."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from simplefe_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "sfe_dsp.h")
EIG_FUNCS = ("sfe_dsp_eig_plan", "sfe_dsp_eig_create", "sfe_dsp_eig_set_steering", "sfe_dsp_eig_set_signal_dim",
             "sfe_dsp_eig_process_stream", "sfe_dsp_eig_destroy")
# (S, B, E, M) the block refuses: each below its range and one above it, and the products above 2^20
BAD_SHAPES = {"S = 0": (0, 1, 0, 1), "S = 65": (65, 1, 0, 1), "negative S": (-1, 1, 0, 1), "B = 65": (1, 65, 0, 1),
              "negative B": (1, -1, 0, 1), "E = S + 1": (4, 1, 5, 1), "negative E": (4, 1, -1, 1), "M = 0": (1, 1, 0, 0),
              "M = 1025": (1, 1, 0, 1025), "negative M": (1, 1, 0, -1), "M B S = 2^20 + 2^14": (64, 64, 0, 260),
              "M E S = 2^20 + 2^12": (64, 0, 64, 257)}
FP = C.POINTER(C.c_float)
N_SCENE = 4096


@pytest.fixture(scope="module")
def L():
    from simplefe_amd import lib
    return lib.load()


def _ones(S, B, M):
    a = np.zeros((max(M, 1), max(B, 1), max(S, 1), 2), np.float32)
    a[..., 0] = 1.0
    return a


def _plan(L, S, B, E, M, a, wl=0, D=0):
    return L.sfe_dsp_eig_plan(S, B, E, M, a.ctypes.data_as(FP) if a is not None else None, wl, D, None, None, None, None, None)


def _create(L, S, B, E, M, a, wl=0, D=0):
    h = C.c_void_p()
    rc = L.sfe_dsp_eig_create(a.ctypes.data_as(FP) if a is not None else None, S, B, E, M, wl, D, 0, C.byref(h))
    return rc, h.value


def _refused(L, S, B, E, M, a, **kw):
    """Plan and create both refuse with an "eig: " message; create does so before it looks for a device."""
    from simplefe_amd import lib
    assert _plan(L, S, B, E, M, a, **kw) == lib.SFE_EINVAL
    assert L.sfe_dsp_last_error().startswith(b"eig: "), L.sfe_dsp_last_error()
    rc, h = _create(L, S, B, E, M, a, **kw)
    assert rc == lib.SFE_EINVAL and not h
    assert L.sfe_dsp_last_error().startswith(b"eig: "), L.sfe_dsp_last_error()


def test_header_declares_eig_abi_and_library_exports_it(L):
    from simplefe_amd import lib
    declared = set(re.findall(r"\b(sfe_dsp_eig_[a-z0-9_]+)\s*\(", open(HDR).read()))
    assert declared == set(EIG_FUNCS)
    for name in EIG_FUNCS:
        assert hasattr(L, name), name
        assert name in lib.SIGNATURES, name


@pytest.mark.parametrize("why", list(BAD_SHAPES))
def test_plan_and_create_refuse_a_bad_shape_with_a_message(L, why):
    S, B, E, M = BAD_SHAPES[why]
    _refused(L, S, B, E, M, _ones(S, B, M))


def test_plan_and_create_refuse_bad_steering_signal_dim_and_mode(L):
    from simplefe_amd import lib
    S, B, E, M = 3, 2, 2, 2
    good = _ones(S, B, M)
    assert _plan(L, S, B, E, M, good, 1, 5) == lib.SFE_OK
    assert _plan(L, S, B, E, M, good, 0, 4) == lib.SFE_OK
    assert _plan(L, S, 0, E, M, None, 0, 0) == lib.SFE_OK            # no beams: no steering wanted
    assert _plan(L, S, 0, 0, M, None, 1, 1) == lib.SFE_OK
    _refused(L, S, B, E, M, None)
    zero = good.copy()
    zero[1, 1] = 0.0                                        # one steering vector all zero
    _refused(L, S, B, E, M, zero)
    assert b"band 1" in L.sfe_dsp_last_error() and b"beam 1" in L.sfe_dsp_last_error()
    for bad in (np.nan, np.inf, -np.inf):
        a = good.copy()
        a[1, 0, 2, 1] = bad
        _refused(L, S, B, E, M, a)
    _refused(L, S, B, E, M, good, wl=2)
    _refused(L, S, B, E, M, good, wl=-1)
    _refused(L, S, B, E, M, good, wl=1, D=6)                # D = 2S
    _refused(L, S, B, E, M, good, wl=1, D=-1)
    _refused(L, S, B, E, M, good, wl=0, D=3)                # odd in the linear mode
    assert b"even" in L.sfe_dsp_last_error()
    _refused(L, S, B, E, M, good, wl=0, D=6)
    # a Gram to decompose needs somewhere to put the eigenvalues
    G = np.eye(2 * S, dtype=np.float32)
    assert L.sfe_dsp_eig_plan(S, 0, 0, 1, None, 0, 0, G.ctypes.data_as(FP), None, None, None, None) == lib.SFE_EINVAL
    assert L.sfe_dsp_last_error().startswith(b"eig: ")


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present: create succeeds there")
def test_create_without_gpu_is_enodev():
    from simplefe_amd import api, lib
    with pytest.raises(lib.SfeError) as e:
        api.Eig(np.ones((2, 4), np.complex64), signal_dim=2)
    assert e.value.code == lib.SFE_ENODEV


_grams = {}


def _scene_gram(S, scene="cov", seed=7):
    key = (S, scene, seed)
    if key not in _grams:
        x, _, _, a = (synth.cov_scene if scene == "cov" else synth.mvdr_scene_rectilinear)(S, N_SCENE, seed)
        G = synth.cov_reference(x, S, 1, N_SCENE, 1.0 / N_SCENE)[0, 0].astype(np.float32)
        G.setflags(write=False)
        _grams[key] = (G, a)
    return _grams[key]


def _steering(S, B, a_d):
    """(B, S) complex64: the scene's own steering vector, then a sine grid of scan directions (test_mvdr_host's)."""
    u = -1.0 + (2.0 * np.arange(B) + 1.0) / B
    st = np.exp(1j * np.pi * u[:, None] * np.arange(S)[None, :])
    st[0] = a_d
    return st.astype(np.complex64)


def _ulps(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    key = lambda v: np.where(v.view(np.int32) < 0, np.int64(-2 ** 31) - v.view(np.int32), v.view(np.int32)).astype(np.int64)
    return int(np.abs(key(a) - key(b)).max())


def _projector(rows):
    r = np.asarray(rows, np.float64)
    return r.T @ r


@pytest.mark.parametrize("wl", [0, 1], ids=["linear", "widely-linear"])
@pytest.mark.parametrize("S", [1, 4, 9])
def test_plan_is_the_reference_rounded_once(S, wl):
    """Two float64 computations of one law (Jacobi here, LAPACK there), each rounded once to float32: eigenvalues within
    4 ulps, null values within 2^-22, the projector of the signal subspace -- the first D rows of the eigen-beams, behind
    which the scenes have a gap; the projector of all 2S rows is the identity whatever they are -- within n 2^-23
    (Frobenius), and the residual max |G^ V - V Lambda| / lambda_0 of all of them within n 2^-23, which ties every vector
    to its eigenvalue.  Two bands (two draws of cov_scene, the second with the beams in another order), three beams."""
    from simplefe_amd import api
    n, E, B = 2 * S, S, 3
    D = 0 if S == 1 else 4
    G = np.stack([_scene_gram(S)[0], _scene_gram(S, seed=8)[0]])
    st = np.stack([_steering(S, B, _scene_gram(S)[1]), _steering(S, B, _scene_gram(S, seed=8)[1])[::-1]])
    val, nul, vec, status = api.eig_plan(st, G, wl, D, E)
    vr, nr, er, sr, _ = synth.eig_reference(G, st, wl, D, E)
    assert val.shape == (2, n) and nul.shape == (2, B) and vec.shape == (2, 2 * E, n) and status.dtype == np.int32
    assert np.array_equal(status, sr) and not status.any()
    assert (np.diff(val, axis=1) <= 0).all()                                    # descending
    assert _ulps(val, vr) <= 4, _ulps(val, vr)
    assert np.abs(nul.astype(np.float64) - nr).max() <= 2.0 ** -22
    assert (nul >= 0).all() and (nul <= 1 + 2.0 ** -22).all()
    for k in range(2):
        assert np.linalg.norm(_projector(vec[k][:D]) - _projector(er[k][:D])) <= n * 2.0 ** -23
        rows = vec[k].astype(np.float64)
        Gh = synth.mvdr_loaded_matrix(G[k], wl)
        assert np.abs(Gh @ rows.T - rows.T * val[k].astype(np.float64)).max() <= n * 2.0 ** -23 * float(val[k, 0])
        assert np.abs(rows @ rows.T - np.eye(2 * E)).max() <= n * 2.0 ** -23     # unit norm, orthogonal
        if wl:      # the sign rule: the first largest component of every vector is positive
            assert (rows[np.arange(2 * E), np.abs(rows).argmax(axis=1)] > 0).all()
    if not wl:      # contract 5 holds for the plan too
        assert np.array_equal(vec[:, 1::2, 0::2], -vec[:, 0::2, 1::2]) and np.array_equal(vec[:, 1::2, 1::2], vec[:, 0::2, 0::2])
        assert np.abs(val[:, 0::2].astype(np.float64) - val[:, 1::2]).max() <= 4 * 2.0 ** -23 * val.max()   # every eigenvalue twice
    # each optional output may be left out, and a handle of no beams and no vectors gives the same eigenvalues
    only = api.eig_plan(None, G, wl, D, 0, n_in=S, n_bands=2)
    assert np.array_equal(only[0].view(np.uint32), val.view(np.uint32)) and only[1].shape == (2, 0) and only[2].shape == (2, 0, n)
    assert api._l.load().sfe_dsp_eig_plan(S, B, E, 2, st.view(np.float32).ctypes.data_as(FP), wl, D, G.ctypes.data_as(FP),
                                          val.ctypes.data_as(FP), None, None, None) == 0


def test_plan_reads_only_the_upper_triangle():
    from simplefe_amd import api
    S = 4
    G, a = _scene_gram(S)
    st = _steering(S, 2, a)
    poisoned = G.copy()
    poisoned[np.tril_indices(2 * S, -1)] = np.nan
    for wl in (0, 1):
        for got, want in zip(api.eig_plan(st, poisoned, wl, 2, S), api.eig_plan(st, G, wl, 2, S)):
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("wl", [0, 1], ids=["linear", "widely-linear"])
def test_a_nan_fails_the_problem_and_gives_the_selection_matrix(wl):
    from simplefe_amd import api
    S, E = 4, 3
    n = 2 * S
    st = _steering(S, 2, _scene_gram(S)[1])
    good = _scene_gram(S)[0]
    for name, at in (("NaN", np.nan), ("inf", np.inf)):
        bad = good.copy()
        bad[2, 5] = at
        G = np.stack([good, bad])
        val, nul, vec, status = api.eig_plan(np.stack([st, st]), G, wl, 2, E)
        assert status.tolist() == [0, 1], name
        assert np.isnan(val[1]).all() and np.isnan(nul[1]).all(), name
        assert np.array_equal(vec[1], np.eye(2 * E, n, dtype=np.float32)), name
        assert np.isfinite(val[0]).all() and np.isfinite(nul[0]).all() and np.isfinite(vec).all(), name
        vr, nr, er, sr, _ = synth.eig_reference(G, np.stack([st, st]), wl, 2, E)
        assert sr.tolist() == [0, 1] and np.isnan(vr[1]).all() and np.isnan(nr[1]).all() and np.array_equal(er[1], np.eye(2 * E, n))


@pytest.mark.parametrize("wl", [0, 1], ids=["linear", "widely-linear"])
def test_plan_is_exact_on_a_diagonal_matrix(wl):
    """Contract 6 on the host: distinct powers of two with a negative one among them, nothing to rotate."""
    from simplefe_amd import api
    S, D = 4, 2
    n = 2 * S
    d = np.array([0.25, -2.0, 8.0, 1.0, 0.5, 16.0, -0.125, 4.0], np.float32)
    if not wl:
        d = np.repeat(d[::2], 2)                            # the linear structure: every entry twice
    st = np.zeros((S, S), np.complex64)
    st[np.arange(S), np.arange(S)] = 1.0                    # selection steering vectors
    val, nul, vec, status = api.eig_plan(st, np.diag(d), wl, D, S)
    order = np.argsort(-d, kind="stable")
    assert status.tolist() == [0] and np.array_equal(val[0], d[order])
    want = np.zeros((n, n), np.float32)
    want[np.arange(n), order] = 1.0
    if not wl:
        want[1::2] = 0.0
        want[np.arange(1, n, 2), order[0::2] ^ 1] = 1.0     # the twin row: the rotation of e_2s is e_2s+1
    assert np.array_equal(vec[0], want)
    signal = set(order[:D] // 2)                            # streams inside the signal subspace: null 0 there, 1 elsewhere
    if wl:      # one dimension of a stream's two may be signal: lambda_min(Q) is the smaller, 0
        want_null = [0.0 if (2 * s in order[:D] or 2 * s + 1 in order[:D]) else 1.0 for s in range(S)]
    else:
        want_null = [0.0 if s in signal else 1.0 for s in range(S)]
    assert nul[0].tolist() == want_null


def _twin_rows(rows):
    """Rows 2e of a real matrix with their exact rotations as rows 2e + 1: the law's step 5."""
    T = np.array(rows, np.float64)
    T[1::2, 0::2], T[1::2, 1::2] = -T[0::2, 1::2], T[0::2, 0::2]
    return T


def test_linear_mode_pairs_are_orthonormal_where_a_real_method_is_not():
    """Why the linear mode rotates the S x S Hermitian matrix.  The Gram of three snapshots of nine streams has a
    12-dimensional null space in the linear mode.  Given the linear mode's G^ as a widely-linear problem, the plan runs
    its real Jacobi method on it and returns a correct orthonormal basis -- but an arbitrary one inside that space, so
    rows 0, 2, 4 ... with their exact rotations are far from orthonormal: no real method can promise otherwise where an
    eigenvalue has more than two dimensions.  The linear mode itself returns exact (u(w), u(jw)) pairs."""
    from simplefe_amd import api
    S = 9
    n = 2 * S
    rng = np.random.default_rng(21)
    x = rng.integers(-3, 4, (S, 3)) + 1j * rng.integers(-3, 4, (S, 3))
    U = synth.cov_columns(x, S, 1)[0]
    G = (U @ U.T).astype(np.float32)                        # small integers: exact
    Gh = synth.mvdr_loaded_matrix(G, False)
    val, _, vec, status = api.eig_plan(None, Gh.astype(np.float32), True, 0, S, n_in=S)
    assert status.tolist() == [0]
    own = vec[0].astype(np.float64)
    assert np.abs(own @ own.T - np.eye(n)).max() <= n * 2.0 ** -23          # the real method's own basis is fine
    twin = _twin_rows(own)
    assert np.abs(twin @ twin.T - np.eye(n)).max() >= 0.1                   # its twin-structured form is not
    val, _, vec, status = api.eig_plan(None, G, False, 0, S, n_in=S)
    assert status.tolist() == [0]
    rows = vec[0].astype(np.float64)
    assert np.array_equal(rows, _twin_rows(rows))
    assert np.abs(rows @ rows.T - np.eye(n)).max() <= n * 2.0 ** -23
    assert np.abs(Gh @ rows.T - rows.T * val[0].astype(np.float64)).max() <= n * 2.0 ** -23 * float(val[0, 0])
    assert np.abs(val[0, 6:]).max() <= n * 2.0 ** -23 * float(val[0, 0])


def _minima(null, k=2):
    """Indices of the k smallest strict local minima of a spectrum over a grid (the ends count)."""
    v = np.concatenate([[np.inf], np.asarray(null, np.float64), [np.inf]])
    at = [i for i in range(null.size) if v[i + 1] < v[i] and v[i + 1] < v[i + 2]]
    return sorted(sorted(at, key=lambda i: null[i])[:k])


def _nearest(S, B, deg):
    """Where on _steering's grid (slot 0 holds the scene's own vector: left out) sin(deg) falls."""
    u = -1.0 + (2.0 * np.arange(B) + 1.0) / B
    return 1 + int(np.abs(u[1:] - np.sin(np.deg2rad(deg))).argmin())


@pytest.mark.parametrize("case", [(4, "cov", 0, 4), (9, "cov", 0, 4), (4, "rect", 1, 3), (9, "rect", 1, 3)],
                         ids=["S4-linear", "S9-linear", "S4-rectilinear-wl", "S9-rectilinear-wl"])
def test_music_finds_both_sources(case):
    """The two smallest local minima of the null spectrum over a 64-point sine grid lie at the grid points nearest the
    signal (10 degrees) and the interferer (-35 degrees); at the true steering vector (slot 0) null is a few 1e-6."""
    from simplefe_amd import api
    S, scene, wl, D = case
    B = 64
    G, a = _scene_gram(S, scene)
    st = _steering(S, B, a)
    val, nul, _, status = api.eig_plan(st, G, wl, D)
    assert status.tolist() == [0]
    grid = nul[0, 1:]
    found = [1 + i for i in _minima(grid)]
    assert found == sorted([_nearest(S, B, 10.0), _nearest(S, B, -35.0)]), (found, grid[np.array(found) - 1])
    assert 0.0 <= nul[0, 0] <= 1e-4
    ref = synth.eig_reference(G, st, wl, D)[1]
    assert np.abs(nul.astype(np.float64) - ref).max() <= 2.0 ** -22


def test_eig_kernels_use_no_scratch():
    from simplefe_amd import build
    res = json.load(open(os.path.join(build.HERE, "build", "eig.hip.resources.json")))
    assert sum("eig_kernel<" in k for k in res) == 2
    for k, r in res.items():
        assert r["ScratchSize"] == 0 and r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0, (k, r)
        assert r["LDS Size"] == 0, (k, r)                   # all of it dynamic: a small problem takes a small share
        assert r["VGPRs"] <= 128, (k, r)                    # two workgroups per SIMD where the LDS allows


def test_eig_sources_are_in_the_build_lists():
    from simplefe_amd import build
    assert "eig.hip" in build.EXACT_SOURCES and "api_eig.hip" in build.HOST_SOURCES
    assert build.KERNEL_FILES["eig"] == ("eig.hip", "eig.h", "common.h")
    assert build.SCRATCH_FREE["eig.hip"] == "eigen-solver"
    cm = open(os.path.join(ROOT, "CMakeLists.txt")).read()
    exact = re.search(r"set\(SFE_EXACT_SOURCES ([^)]*)\)", cm).group(1).split()
    assert sorted(exact) == sorted(build.EXACT_SOURCES)
