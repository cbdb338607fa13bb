"""The streaming spatial covariance estimator (sfe_dsp_cov_*) without a GPU: the C ABI's declarations and exports, the
host-only planner and its refusals, the no-GPU refusal, the float64 references the GPU tests compare against
(synth.cov_reference, cov_from_gram, mvdr_weights, cov_scene), and the kernels' register budget."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from simplefe_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "sfe_dsp.h")
COV_FUNCS = ("sfe_dsp_cov_plan", "sfe_dsp_cov_create", "sfe_dsp_cov_set_input_format", "sfe_dsp_cov_process_stream",
             "sfe_dsp_cov_reset", "sfe_dsp_cov_destroy")
# (S, M, A) the block refuses: each of the three at 0, negative and one above its limit, and A off the chunk grid
BAD_SHAPES = {"S = 0": (0, 1, 64), "S = 65": (65, 1, 64), "negative S": (-1, 1, 64), "M = 0": (1, 0, 64), "M = 1025": (1, 1025, 64),
              "A = 0": (1, 1, 0), "negative A": (1, 1, -64), "A = 1": (1, 1, 1), "A = T - 1": (1, 1, 63), "A = T + 1": (1, 1, 65),
              "A = 2^24 + T": (1, 1, (1 << 24) + 64), "A = 3 2^23": (1, 1, 3 << 23)}


@pytest.fixture(scope="module")
def L():
    from simplefe_amd import lib
    return lib.load()


def _plan(L, S, M, A):
    t, c = C.c_int(-1), C.c_int(-1)
    return L.sfe_dsp_cov_plan(S, M, A, C.byref(t), C.byref(c)), t.value, c.value


def test_header_declares_cov_abi_and_library_exports_it(L):
    from simplefe_amd import lib
    declared = set(re.findall(r"\b(sfe_dsp_cov_[a-z0-9_]+)\s*\(", open(HDR).read()))
    assert declared == set(COV_FUNCS)
    for name in COV_FUNCS:
        assert hasattr(L, name), name
        assert name in lib.SIGNATURES, name


def test_plan_reports_one_chunk_for_every_shape_and_the_smallest_group(L):
    from simplefe_amd import api, lib
    rc, T, _ = _plan(L, 1, 1, 1 << 24)
    assert rc == lib.SFE_OK and 16 <= T <= 256 and T & (T - 1) == 0
    for S in (1, 8, 64):
        for M in (1, 1024):
            for chunks in (1, 2, 4, 5, 16, 17, (1 << 24) // T):
                rc, t, c = _plan(L, S, M, chunks * T)
                assert rc == lib.SFE_OK and t == T, (S, M, chunks)
                assert c >= 1 and c & (c - 1) == 0 and c * c >= chunks and (c == 1 or (c // 2) ** 2 < chunks), (chunks, c)
                assert api.cov_plan(S, M, chunks * T) == (T, c)
    assert L.sfe_dsp_cov_plan(64, 1024, 1 << 24, None, None) == lib.SFE_OK     # either output pointer may be null


@pytest.mark.parametrize("why", list(BAD_SHAPES))
def test_plan_and_create_refuse_a_bad_shape_with_a_message(L, why):
    from simplefe_amd import lib
    S, M, A = BAD_SHAPES[why]
    assert _plan(L, S, M, A)[0] == lib.SFE_EINVAL, why
    assert L.sfe_dsp_last_error().startswith(b"cov: "), L.sfe_dsp_last_error()
    h = C.c_void_p()
    assert L.sfe_dsp_cov_create(S, M, A, 1.0, 0, C.byref(h)) == lib.SFE_EINVAL, why       # before it looks for a device
    assert L.sfe_dsp_last_error().startswith(b"cov: ") and not h.value


@pytest.mark.parametrize("scale", [np.nan, np.inf, -np.inf])
def test_create_refuses_a_scale_that_is_not_finite(L, scale):
    from simplefe_amd import lib
    h = C.c_void_p()
    assert L.sfe_dsp_cov_create(4, 1, 64, scale, 0, C.byref(h)) == lib.SFE_EINVAL
    assert L.sfe_dsp_last_error().startswith(b"cov: ") and not h.value


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present: create succeeds there")
def test_create_without_gpu_is_enodev():
    from simplefe_amd import api, lib
    with pytest.raises(lib.SfeError) as e:
        api.Cov(4, 1, 64)
    assert e.value.code == lib.SFE_ENODEV


def test_reference_is_the_gram_of_the_real_columns():
    S, M, A, n = 3, 2, 8, 20                     # two rows and four instants that complete none
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((S, M, n)) + 1j * rng.standard_normal((S, M, n))).astype(np.complex64)
    G = synth.cov_reference(x, S, M, A, 0.25)
    assert G.shape == (M, 2, 2 * S, 2 * S) and G.dtype == np.float64
    u = np.stack([x.real, x.imag], axis=1).reshape(2 * S, M, n).astype(np.float64)     # row 2s: Re x_s, row 2s+1: Im x_s
    for r in range(2):
        want = 0.25 * np.einsum("ikm,jkm->kij", u[:, :, r * A:(r + 1) * A], u[:, :, r * A:(r + 1) * A])
        assert np.abs(G[:, r] - want).max() <= 1e-13 * np.abs(want).max()
    assert np.array_equal(synth.cov_reference(x[:, 1], S, 1, A, 0.25)[0], G[1])         # one band, two-dimensional


def test_covariance_and_pseudo_covariance_come_out_of_the_gram():
    S, n = 4, 64
    rng = np.random.default_rng(4)
    x = rng.standard_normal((S, n)) + 1j * rng.standard_normal((S, n))
    Cm, Pm = synth.cov_from_gram(synth.cov_reference(x, S, 1, n, 1.0)[0, 0])
    assert Cm.dtype == Pm.dtype == np.complex128
    assert np.abs(Cm - x @ x.conj().T).max() <= 1e-12 * n and np.abs(Pm - x @ x.T).max() <= 1e-12 * n


def test_mvdr_weights_have_unit_response_on_their_steering_vector():
    S, n = 4, 4096
    x, x_d, x_i, a = synth.cov_scene(S, n, 7)
    assert x.shape == x_d.shape == x_i.shape == (S, n) and x.dtype == np.complex64
    assert abs(np.abs(x).max() - 0.9) < 1e-6
    sir_in = 10 * np.log10((np.abs(x_d) ** 2).sum() / (np.abs(x_i) ** 2).sum())
    assert abs(sir_in + 30.0) < 0.5, sir_in
    Cm, _ = synth.cov_from_gram(synth.cov_reference(x, S, 1, n, 1.0 / n)[0, 0])
    for loading in (0.0, 1e-6, 1e-2):
        W = synth.mvdr_weights(Cm, a, loading)
        assert W.shape == (1, 1, S) and W.dtype == np.complex64
        assert abs(W[0, 0].astype(np.complex128) @ a - 1.0) < 1e-6
    w = synth.mvdr_weights(Cm, a, 1e-6)[0, 0].astype(np.complex128)
    sir_out = 10 * np.log10((np.abs(w @ x_d) ** 2).sum() / (np.abs(w @ x_i) ** 2).sum())
    assert sir_out >= 40.0, sir_out


def test_cov_kernels_use_no_scratch():
    from simplefe_amd import build
    res = json.load(open(os.path.join(build.HERE, "build", "cov.hip.resources.json")))
    kernels = {k: r for k, r in res.items() if "cov_chunk_kernel<" in k}
    classes = {tuple(a.strip() for a in re.search(r"cov_chunk_kernel<(.*?)>", k).group(1).split(",")) for k in kernels}
    assert classes == {(str(nt), u8) for nt in range(1, 9) for u8 in ("true", "false")}
    assert any("cov_row_kernel" in k for k in res)
    for k, r in res.items():
        assert r["ScratchSize"] == 0 and r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0, (k, r)
        assert r["LDS Size"] <= 65536, (k, r)


def test_cov_sources_are_in_the_build_lists():
    from simplefe_amd import build
    assert "cov.hip" in build.EXACT_SOURCES and "api_cov.hip" in build.HOST_SOURCES
    assert build.KERNEL_FILES["cov"] == ("cov.hip", "cov.h", "common.h")
    assert build.SCRATCH_FREE["cov.hip"] == "covariance"
    cm = open(os.path.join(ROOT, "CMakeLists.txt")).read()
    assert re.search(r"set\(SFE_EXACT_SOURCES [^)]*\bcov\.hip\b", cm)
