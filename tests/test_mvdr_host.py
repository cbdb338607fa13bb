"""The adaptive beamforming weight solver (sfe_dsp_mvdr_*) without a GPU: the C ABI's declarations and exports, the
host-only planner -- its refusals, its float64 solve against the independent numpy statement of the law
(synth.mvdr_reference), its failure paths -- the no-GPU refusal, the reference against the project's older
synth.mvdr_weights, the build lists and the kernels' register budget."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from simplefe_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "sfe_dsp.h")
MVDR_FUNCS = ("sfe_dsp_mvdr_plan", "sfe_dsp_mvdr_create", "sfe_dsp_mvdr_set_steering", "sfe_dsp_mvdr_set_loading",
              "sfe_dsp_mvdr_process_stream", "sfe_dsp_mvdr_load_beam", "sfe_dsp_mvdr_destroy")
# (S, B, M) the block refuses: each at 0, negative and one above its limit, and the product above 2^20
BAD_SHAPES = {"S = 0": (0, 1, 1), "S = 65": (65, 1, 1), "negative S": (-1, 1, 1), "B = 0": (1, 0, 1), "B = 65": (1, 65, 1),
              "negative B": (1, -2, 1), "M = 0": (1, 1, 0), "M = 1025": (1, 1, 1025), "negative M": (1, 1, -1),
              "M B S = 2^20 + 2^14": (64, 64, 260)}
FP = C.POINTER(C.c_float)


@pytest.fixture(scope="module")
def L():
    from simplefe_amd import lib
    return lib.load()


def _ones(S, B, M):
    a = np.zeros((max(M, 1), max(B, 1), max(S, 1), 2), np.float32)
    a[..., 0] = 1.0
    return a


def _plan(L, S, B, M, a, wl=0, lr=0.0, la=0.0):
    return L.sfe_dsp_mvdr_plan(S, B, M, a.ctypes.data_as(FP) if a is not None else None, wl, lr, la, None, None, None, None)


def _create(L, S, B, M, a, wl=0, lr=0.0, la=0.0):
    h = C.c_void_p()
    rc = L.sfe_dsp_mvdr_create(a.ctypes.data_as(FP) if a is not None else None, S, B, M, wl, lr, la, 0, C.byref(h))
    return rc, h.value


def _refused(L, S, B, M, a, **kw):
    """Plan and create both refuse with a "mvdr: " message; create does so before it looks for a device."""
    from simplefe_amd import lib
    assert _plan(L, S, B, M, a, **kw) == lib.SFE_EINVAL
    assert L.sfe_dsp_last_error().startswith(b"mvdr: "), L.sfe_dsp_last_error()
    rc, h = _create(L, S, B, M, a, **kw)
    assert rc == lib.SFE_EINVAL and not h
    assert L.sfe_dsp_last_error().startswith(b"mvdr: "), L.sfe_dsp_last_error()


def test_header_declares_mvdr_abi_and_library_exports_it(L):
    from simplefe_amd import lib
    declared = set(re.findall(r"\b(sfe_dsp_mvdr_[a-z0-9_]+)\s*\(", open(HDR).read()))
    assert declared == set(MVDR_FUNCS)
    for name in MVDR_FUNCS:
        assert hasattr(L, name), name
        assert name in lib.SIGNATURES, name


@pytest.mark.parametrize("why", list(BAD_SHAPES))
def test_plan_and_create_refuse_a_bad_shape_with_a_message(L, why):
    S, B, M = BAD_SHAPES[why]
    _refused(L, S, B, M, _ones(S, B, M))


def test_plan_and_create_refuse_bad_steering_loading_and_mode(L):
    from simplefe_amd import lib
    S, B, M = 3, 2, 2
    good = _ones(S, B, M)
    assert _plan(L, S, B, M, good, 1, 1e-3, 1e-9) == lib.SFE_OK
    _refused(L, S, B, M, None)
    zero = good.copy()
    zero[1, 1] = 0.0                                        # one steering vector all zero
    _refused(L, S, B, M, zero)
    assert b"band 1" in L.sfe_dsp_last_error() and b"beam 1" in L.sfe_dsp_last_error()
    for bad in (np.nan, np.inf, -np.inf):
        a = good.copy()
        a[1, 0, 2, 1] = bad
        _refused(L, S, B, M, a)
        _refused(L, S, B, M, good, lr=bad)
        _refused(L, S, B, M, good, la=bad)
    _refused(L, S, B, M, good, lr=-1e-6)
    _refused(L, S, B, M, good, la=-1e-30)
    _refused(L, S, B, M, good, wl=2)
    _refused(L, S, B, M, good, wl=-1)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present: create succeeds there")
def test_create_without_gpu_is_enodev():
    from simplefe_amd import api, lib
    with pytest.raises(lib.SfeError) as e:
        api.Mvdr(np.ones((2, 4), np.complex64), load_rel=1e-4)
    assert e.value.code == lib.SFE_ENODEV


def _scene_gram(S, seed=7, n=4096):
    x, _, _, a = synth.cov_scene(S, n, seed)
    return synth.cov_reference(x, S, 1, n, 1.0 / n)[0, 0].astype(np.float32), a


def _steering(S, B, a_d):
    """(B, S) complex64: the scene's own steering vector, then a sine grid of scan directions."""
    u = -1.0 + (2.0 * np.arange(B) + 1.0) / B
    st = np.exp(1j * np.pi * u[:, None] * np.arange(S)[None, :])
    st[0] = a_d
    return st.astype(np.complex64)


def _ulps(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    key = lambda v: np.where(v.view(np.int32) < 0, np.int64(-2 ** 31) - v.view(np.int32), v.view(np.int32)).astype(np.int64)
    return int(np.abs(key(a) - key(b)).max())


@pytest.mark.parametrize("wl", [0, 1], ids=["linear", "widely-linear"])
@pytest.mark.parametrize("S", [1, 4, 9])
def test_plan_is_the_reference_rounded_once(S, wl):
    """Two float64 computations of one law, each rounded once to float32: 4 ulps per entry.  Two bands (two draws of
    cov_scene, the second with the beams in another order), three beams, both loadings at once."""
    from simplefe_amd import api
    G0, a0 = _scene_gram(S)
    G1, a1 = _scene_gram(S, seed=8)
    G = np.stack([G0, G1])
    st = np.stack([_steering(S, 3, a0), _steering(S, 3, a1)[::-1]])
    R, pw, status = api.mvdr_plan(st, G, wl, 1e-4, 1e-7)
    Rr, pr, sr = synth.mvdr_reference(G, st, wl, 1e-4, 1e-7)
    assert R.shape == (2, 6, 2 * S) and pw.shape == (2, 3) and status.dtype == np.int32
    assert np.array_equal(status, sr) and not status.any()
    assert np.isfinite(R).all() and (pw > 0).all()
    assert _ulps(R, Rr) <= 4 and _ulps(pw, pr) <= 4, (_ulps(R, Rr), _ulps(pw, pr))
    # unit response on the steering vector: R_b A2 = I_2
    for k in range(2):
        for b in range(3):
            assert np.abs(Rr[k, 2 * b:2 * b + 2] @ synth.mvdr_rhs(st[k, b]) - np.eye(2)).max() < 1e-9
    if not wl:          # contract 4 holds for the plan too
        assert np.array_equal(R[:, 1::2, 0::2], -R[:, 0::2, 1::2]) and np.array_equal(R[:, 1::2, 1::2], R[:, 0::2, 0::2])
    # each output may be left out
    assert api._l.load().sfe_dsp_mvdr_plan(S, 3, 2, st.view(np.float32).ctypes.data_as(FP), wl, 1e-4, 0.0,
                                           G.ctypes.data_as(FP), None, None, None) == 0


def test_plan_reads_only_the_upper_triangle():
    from simplefe_amd import api
    S = 4
    G, a = _scene_gram(S)
    st = _steering(S, 2, a)
    poisoned = G.copy()
    poisoned[np.tril_indices(2 * S, -1)] = np.nan
    for wl in (0, 1):
        for got, want in zip(api.mvdr_plan(st, poisoned, wl, 1e-3), api.mvdr_plan(st, G, wl, 1e-3)):
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("S", [4, 9, 16, 64])
def test_linear_reference_is_the_older_mvdr_weights(S):
    """synth.mvdr_weights (complex, numpy solve, complex64 result) through sfe_dsp_beam_plan's real matrix."""
    from simplefe_amd import api
    G, a = _scene_gram(S)
    a = a.astype(np.complex64)
    Cm, _ = synth.cov_from_gram(G)
    for lr in (1e-4, 1e-2):
        Rw = api.beam_plan(synth.mvdr_weights(Cm, a, lr)).astype(np.float64)
        Rr, pr, _ = synth.mvdr_reference(G, a[None, :], False, lr, 0.0)
        assert np.linalg.norm(Rw - Rr) <= 1e-6 * np.linalg.norm(Rr)
        a64 = a.astype(np.complex128)
        Cl = Cm + lr * np.trace(Cm).real / S * np.eye(S)
        assert abs(pr[0, 0] * (a64.conj() @ np.linalg.solve(Cl, a64)).real - 1.0) < 1e-9      # power = 1 / (a^H C^-1 a)
        # and trace(Q^-1) of the widely-linear form on a circular matrix is the same number
        Gl = synth.mvdr_loaded_matrix(G, False, lr)
        A2 = synth.mvdr_rhs(a)
        assert abs(np.trace(np.linalg.inv(A2.T @ np.linalg.solve(Gl, A2))) / pr[0, 0] - 1.0) < 1e-9


@pytest.mark.parametrize("wl", [0, 1], ids=["linear", "widely-linear"])
def test_failed_factorisation_gives_the_conventional_beamformer(wl):
    from simplefe_amd import api
    S = 4
    rng = np.random.default_rng(5)
    st = (rng.standard_normal((2, S)) + 1j * rng.standard_normal((2, S))).astype(np.complex64)
    n = 2 * S
    nan = np.eye(n, dtype=np.float32)
    nan[2, 5] = np.nan
    want = api.beam_plan((st.astype(np.complex128).conj() / (np.abs(st.astype(np.complex128)) ** 2).sum(axis=1, keepdims=True))[None])
    for name, G in (("zero", np.zeros((n, n), np.float32)), ("-I", -np.eye(n, dtype=np.float32)), ("NaN", nan)):
        R, pw, status = api.mvdr_plan(st, G, wl, 0.0, 0.0)
        assert status.tolist() == [1], name
        assert np.isnan(pw).all(), name
        assert np.isfinite(R).all() and _ulps(R, want) <= 1, name          # conj(a) / |a|^2, V = 0
        assert _ulps(R, synth.mvdr_fallback(st)) <= 1, name
        Rr, pr, sr = synth.mvdr_reference(G, st, wl, 0.0, 0.0)
        assert sr.tolist() == [1] and np.isnan(pr).all()
    # loading rescues the zero matrix and nothing rescues the NaN
    assert api.mvdr_plan(st, np.zeros((n, n), np.float32), wl, 0.0, 1.0)[2].tolist() == [0]
    assert api.mvdr_plan(st, nan, wl, 1.0, 1.0)[2].tolist() == [1]


def test_rectilinear_scene_has_a_pseudo_covariance():
    S, n = 2, 4096
    x, x_d, x_i, a = synth.mvdr_scene_rectilinear(S, n, 7)
    assert x.shape == x_d.shape == x_i.shape == (S, n) and x.dtype == np.complex64 and abs(np.abs(x).max() - 0.9) < 1e-6
    assert abs(10 * np.log10((np.abs(x_d) ** 2).sum() / (np.abs(x_i) ** 2).sum()) + 30.0) < 0.5
    Cm, Pm = synth.cov_from_gram(synth.cov_reference(x, S, 1, n, 1.0 / n)[0, 0])
    assert np.abs(Pm).max() > 0.9 * np.abs(Cm).max()                        # cov_scene's is ~ 1/sqrt(n) of it
    Cc, Pc = synth.cov_from_gram(synth.cov_reference(synth.cov_scene(S, n, 7)[0], S, 1, n, 1.0 / n)[0, 0])
    assert np.abs(Pc).max() < 0.1 * np.abs(Cc).max()


def test_mvdr_kernels_use_no_scratch():
    from simplefe_amd import build
    res = json.load(open(os.path.join(build.HERE, "build", "mvdr.hip.resources.json")))
    assert sum("mvdr_kernel<" in k for k in res) == 2 and any("mvdr_load_beam_kernel" in k for k in res)
    for k, r in res.items():
        assert r["ScratchSize"] == 0 and r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0, (k, r)
        assert r["LDS Size"] <= 65536, (k, r)


def test_mvdr_sources_are_in_the_build_lists():
    from simplefe_amd import build
    assert "mvdr.hip" in build.EXACT_SOURCES and "api_mvdr.hip" in build.HOST_SOURCES and "beam_view.h" in build.HOST_SOURCES
    assert build.KERNEL_FILES["mvdr"] == ("mvdr.hip", "mvdr.h", "beam.h", "common.h")
    assert build.SCRATCH_FREE["mvdr.hip"] == "weight-solver"
    cm = open(os.path.join(ROOT, "CMakeLists.txt")).read()
    exact = re.search(r"set\(SFE_EXACT_SOURCES ([^)]*)\)", cm).group(1).split()
    assert sorted(exact) == sorted(build.EXACT_SOURCES)
    # the accessor the hand-over uses is internal: no new sfe_dsp_beam_* name, and the kernels' beam files are untouched
    hdr = open(HDR).read()
    assert "sfe_dsp_beam_view" not in hdr and "beam_view" not in hdr
