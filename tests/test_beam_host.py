"""The multi-stream beamformer / stream-mixing bank (sfe_dsp_beam_*) without a GPU: the C ABI's declarations and exports,
the host-only planner, its refusals and its real matrices against their numpy twin (synth.beam_real_matrix), the no-GPU
refusal, the float64 reference the GPU tests compare against, and the kernels' register budget."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from simplefe_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "sfe_dsp.h")
BEAM_FUNCS = ("sfe_dsp_beam_plan", "sfe_dsp_beam_create", "sfe_dsp_beam_set_input_format", "sfe_dsp_beam_set_weights",
              "sfe_dsp_beam_process_stream", "sfe_dsp_beam_destroy")
FP = C.POINTER(C.c_float)
# (S, B, M) the block refuses whatever the weights hold: each of the three at 0 and one above its limit, and M B S > 2^20
BAD_SHAPES = {"S = 0": (0, 1, 1), "B = 0": (1, 0, 1), "M = 0": (1, 1, 0), "S = 65": (65, 1, 1), "B = 65": (1, 65, 1),
              "M = 1025": (1, 1, 1025), "M B S = 2^20 + 1024": (32, 33, 1024), "negative S": (-1, 1, 1)}
BAD_VALUES = {"NaN in W": ("w", np.nan), "Inf in W": ("w", np.inf), "-Inf in W": ("w", -np.inf), "NaN in V": ("v", np.nan),
              "Inf in V": ("v", np.inf)}
SHAPES = [(1, 1, 1), (3, 2, 1), (5, 7, 4)]


@pytest.fixture(scope="module")
def L():
    from simplefe_amd import lib
    return lib.load()


def _weights(S, B, M, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((M, B, S)) + 1j * rng.standard_normal((M, B, S))).astype(np.complex64)


def _ptr(a):
    return None if a is None else a.view(np.float32).ctypes.data_as(FP)


def test_header_declares_beam_abi_and_library_exports_it(L):
    from simplefe_amd import lib
    declared = set(re.findall(r"\b(sfe_dsp_beam_[a-z0-9_]+)\s*\(", open(HDR).read()))
    assert declared == set(BEAM_FUNCS)
    for name in BEAM_FUNCS:
        assert hasattr(L, name), name
        assert name in lib.SIGNATURES, name


def _bad_value_args(why):
    which, val = BAD_VALUES[why]
    S, B, M = 3, 2, 2
    w, v = _weights(S, B, M, 1), _weights(S, B, M, 2)
    (w if which == "w" else v).view(np.float32).reshape(-1)[-3] = val          # late in the table: every weight is looked at
    return S, B, M, w, v


@pytest.mark.parametrize("why", list(BAD_SHAPES))
def test_plan_refuses_a_bad_shape_with_a_message(L, why):
    from simplefe_amd import lib
    w = _weights(1, 1, 1, 0)                # never read: the shape is refused first
    S, B, M = BAD_SHAPES[why]
    assert L.sfe_dsp_beam_plan(S, B, M, _ptr(w), None, None) == lib.SFE_EINVAL, why
    assert L.sfe_dsp_last_error().startswith(b"beam: "), L.sfe_dsp_last_error()


@pytest.mark.parametrize("why", list(BAD_VALUES))
def test_plan_refuses_a_non_finite_weight_with_a_message(L, why):
    from simplefe_amd import lib
    S, B, M, w, v = _bad_value_args(why)
    assert L.sfe_dsp_beam_plan(S, B, M, _ptr(w), _ptr(v), None) == lib.SFE_EINVAL, why
    assert L.sfe_dsp_last_error().startswith(b"beam: "), L.sfe_dsp_last_error()


def test_plan_accepts_the_limits(L):
    from simplefe_amd import lib
    for S, B, M in ((64, 64, 256), (1, 1, 1024), (32, 32, 1024)):       # the last: M B S = 2^20 exactly
        w = np.zeros((M, B, S), np.complex64)
        assert L.sfe_dsp_beam_plan(S, B, M, _ptr(w), None, None) == lib.SFE_OK, (S, B, M)


@pytest.mark.parametrize("why", list(BAD_SHAPES) + list(BAD_VALUES))
def test_create_refuses_before_it_looks_for_a_device(L, why):
    from simplefe_amd import lib
    if why in BAD_SHAPES:
        (S, B, M), w, v = BAD_SHAPES[why], _weights(1, 1, 1, 0), None
    else:
        S, B, M, w, v = _bad_value_args(why)
    h = C.c_void_p()
    assert L.sfe_dsp_beam_create(_ptr(w), _ptr(v), S, B, M, 0, C.byref(h)) == lib.SFE_EINVAL, why
    assert L.sfe_dsp_last_error().startswith(b"beam: ") and not h.value


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present: create succeeds there")
def test_create_without_gpu_is_enodev(L):
    from simplefe_amd import api, lib
    with pytest.raises(lib.SfeError) as e:
        api.Beam(synth.beam_steering_weights(4, 2))
    assert e.value.code == lib.SFE_ENODEV


@pytest.mark.parametrize("with_v", [False, True], ids=["V absent", "V present"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_plan_real_matrix_is_the_numpy_twin(L, shape, with_v):
    from simplefe_amd import api
    S, B, M = shape
    w = _weights(S, B, M, 10 + S)
    v = _weights(S, B, M, 20 + S) if with_v else None
    R = api.beam_plan(w, v)
    twin = synth.beam_real_matrix(w, v)
    assert R.shape == twin.shape == (M, 2 * B, 2 * S) and R.dtype == twin.dtype == np.float32
    assert np.array_equal(R.view(np.uint32), twin.view(np.uint32))
    # each entry is the float64 sum rounded once
    v0 = np.zeros_like(w) if v is None else v
    wr, wi, vr, vi = (a.astype(np.float64) for a in (w.real, w.imag, v0.real, v0.imag))
    assert np.array_equal(R[:, 0::2, 0::2], (wr + vr).astype(np.float32))
    assert np.array_equal(R[:, 0::2, 1::2], (-wi + vi).astype(np.float32))
    assert np.array_equal(R[:, 1::2, 0::2], (wi + vi).astype(np.float32))
    assert np.array_equal(R[:, 1::2, 1::2], (wr - vr).astype(np.float32))


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_without_v_the_entries_are_w_own_floats(L, shape):
    from simplefe_amd import api
    S, B, M = shape
    w = _weights(S, B, M, 30 + S)
    w[0, 0, 0] = 1.0 + 0.0j                 # a zero imaginary part: its negation is -0.0, bitwise
    R = api.beam_plan(w)
    u = lambda a: np.ascontiguousarray(a).view(np.uint32)
    assert np.array_equal(u(R[:, 0::2, 0::2]), u(w.real))
    assert np.array_equal(u(R[:, 0::2, 1::2]), u(-w.imag))
    assert np.array_equal(u(R[:, 1::2, 0::2]), u(w.imag))
    assert np.array_equal(u(R[:, 1::2, 1::2]), u(w.real))


@pytest.mark.parametrize("with_v", [False, True], ids=["V absent", "V present"])
def test_reference_is_the_widely_linear_law(with_v):
    """beam_reference against a plain float64 einsum on (W, V).  The weights are multiples of 2^-8 below 4 in magnitude,
    so W + V and W - V are exact in float32 and the rounded R IS the law's matrix: what is left is float64 rounding of
    two different summation orders, 1e-12 relative."""
    S, B, M, n = 5, 7, 4, 257
    rng = np.random.default_rng(5)
    q = lambda: (rng.integers(-512, 512, (M, B, S)) + 1j * rng.integers(-512, 512, (M, B, S))) / 256.0
    w, v = q().astype(np.complex64), (q().astype(np.complex64) if with_v else None)
    x = np.stack([synth.synth_cf32(M * n, ch=s).view(np.complex64).reshape(M, n) for s in range(S)])      # (S, M, n)
    got = synth.beam_reference(x, w, v)
    want = np.einsum("kbs,skm->bkm", w.astype(np.complex128), x.astype(np.complex128))
    if with_v:
        want = want + np.einsum("kbs,skm->bkm", v.astype(np.complex128), np.conj(x.astype(np.complex128)))
    assert got.shape == (B, M, n) and got.dtype == np.complex128
    scale = np.abs(want).max()
    assert np.abs(got - want).max() <= 1e-12 * scale
    # one band, two-dimensional arguments
    assert np.array_equal(synth.beam_reference(x[:, 2], w[2], None if v is None else v[2]), got[:, 2])
    # the float32 yardstick is a float32 product of the same matrix
    y32 = synth.beam_reference(x, w, v, np.float32)
    assert y32.dtype == np.complex64 and synth.rel_rms(y32.view(np.float32), got.astype(np.complex64).view(np.float32)) < 1e-6


def test_steering_weights_point_where_they_say():
    S, B = 8, 4
    w = synth.beam_steering_weights(S, B)
    assert w.shape == (B, S) and w.dtype == np.complex64
    u = -1.0 + (2.0 * np.arange(B) + 1.0) / B
    a = np.exp(1j * np.pi * np.arange(S)[None, :] * u[:, None])         # the array's response to a wave from u_b
    g = w.astype(np.complex128) @ a.T                                   # [beam][direction]
    assert np.allclose(np.diag(g), 1.0, atol=1e-6)
    assert (np.abs(g - np.diag(np.diag(g))) < 0.5).all()


def test_beam_kernels_use_no_scratch():
    from simplefe_amd import build
    res = json.load(open(os.path.join(build.HERE, "build", "beam.hip.resources.json")))
    kernels = {k: r for k, r in res.items() if "beam_kernel<" in k}
    classes = {tuple(a.strip() for a in re.search(r"beam_kernel<(.*?)>", k).group(1).split(",")) for k in kernels}
    assert classes == {(str(kp), str(rt), u8) for kp in (1, 2, 4, 8, 16) for rt in (1, 2, 4, 8) for u8 in ("true", "false")}
    for k, r in kernels.items():
        assert r["ScratchSize"] == 0 and r.get("VGPRs Spill", 0) == 0 and r.get("SGPRs Spill", 0) == 0, (k, r)
        assert r["LDS Size"] <= 65536, (k, r)


def test_beam_sources_are_in_the_build_lists():
    from simplefe_amd import build
    assert "beam.hip" in build.EXACT_SOURCES and "api_beam.hip" in build.HOST_SOURCES
    assert build.KERNEL_FILES["beam"] == ("beam.hip", "beam.h", "common.h")
    assert build.SCRATCH_FREE["beam.hip"] == "beamformer"
    cm = open(os.path.join(ROOT, "CMakeLists.txt")).read()
    assert re.search(r"set\(SFE_EXACT_SOURCES [^)]*\bbeam\.hip\b", cm)
