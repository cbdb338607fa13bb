"""The streaming biquad-cascade IIR filter (sfe_dsp_iir_*) without a GPU: the C ABI's declarations and exports, the
host-only planner and its refusals, the no-GPU refusal, the numpy references the GPU tests compare against (and the
cap on the float32 yardstick that their bars are multiples of), and the kernels' register budget."""
import json
import os
import re

import numpy as np
import pytest

from simplefe_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "sfe_dsp.h")
IIR_FUNCS = ("sfe_dsp_iir_plan", "sfe_dsp_iir_create", "sfe_dsp_iir_set_input_format", "sfe_dsp_iir_process_stream",
             "sfe_dsp_iir_reset", "sfe_dsp_iir_destroy")
FILTERS = synth.iir_grid_filters()
# a section that is stable in float64 and not once rounded: -(1 - 2^-30) rounds to -1.0f
REFUSED = {"no section": np.zeros((0, 6)), "nine sections": np.tile(synth.iir_one_pole(0.5), (9, 1)),
           "a NaN": [[1, 0, float("nan"), 1, -0.5, 0]], "a0 = 0": [[1, 0, 0, 0, -0.5, 0]], "a pole at 1": [[1, 0, 0, 1, -1, 0]],
           "poles on the circle": [[1, 0, 0, 1, 0, 1]], "stable only in float64": [[1, 0, 0, 1, -(1 - 2.0 ** -30), 0]]}


@pytest.fixture(scope="module")
def L():
    from simplefe_amd import lib
    return lib.load()


def test_header_declares_iir_abi_and_library_exports_it(L):
    from simplefe_amd import lib
    declared = set(re.findall(r"\b(sfe_dsp_iir_[a-z0-9_]+)\s*\(", open(HDR).read()))
    assert declared == set(IIR_FUNCS)
    for name in IIR_FUNCS:
        assert hasattr(L, name), name
        assert name in lib.SIGNATURES, name


@pytest.mark.parametrize("name", list(FILTERS))
def test_plan_accepts_the_grid_filters(L, name):
    from simplefe_amd import api
    sos = FILTERS[name]
    G, state = api.iir_plan(sos)
    assert 1024 <= G <= 65536 and G & (G - 1) == 0
    assert state == 6 * len(sos)
    assert G == api.iir_plan(synth.iir_one_pole(0.5))[0]            # the same for every S


def _plan_raw(L, sos, n_sections):
    import ctypes as C
    a = np.ascontiguousarray(np.asarray(sos, dtype=np.float64).reshape(-1))
    if a.size == 0:
        a = np.zeros(6)
    return L.sfe_dsp_iir_plan(a.ctypes.data_as(C.POINTER(C.c_double)), n_sections, None, None)


@pytest.mark.parametrize("why", list(REFUSED))
def test_plan_refuses_with_a_message(L, why):
    from simplefe_amd import lib
    sos = np.asarray(REFUSED[why], dtype=np.float64).reshape(-1, 6)
    assert _plan_raw(L, sos, len(sos)) == lib.SFE_EINVAL, why
    assert L.sfe_dsp_last_error().startswith(b"iir: "), L.sfe_dsp_last_error()


def test_the_stability_test_is_on_the_rounded_values(L):
    from simplefe_amd import api
    a1 = -(1 - 2.0 ** -30)
    assert abs(a1) < 1.0 and np.float32(a1) == np.float32(-1.0)
    assert api.iir_plan([[1, 0, 0, 1, -(1 - 2.0 ** -20), 0]])[0] > 0        # this one survives the rounding
    # a row given with a0 != 1 is normalised first: the same filter, the same verdict
    assert api.iir_plan([[2, 0, 0, 2, -1.99, 0]])[0] > 0
    from simplefe_amd import lib
    with pytest.raises(lib.SfeError):
        api.iir_plan([[2, 0, 0, 2, -2, 0]])


@pytest.mark.parametrize("why", list(REFUSED))
def test_create_refuses_before_it_looks_for_a_device(L, why):
    import ctypes as C
    from simplefe_amd import lib
    sos = np.asarray(REFUSED[why], dtype=np.float64).reshape(-1, 6)
    a = np.ascontiguousarray(sos.reshape(-1)) if sos.size else np.zeros(6)
    h = C.c_void_p()
    assert L.sfe_dsp_iir_create(a.ctypes.data_as(C.POINTER(C.c_double)), len(sos), 1, 1, 0, C.byref(h)) == lib.SFE_EINVAL
    assert L.sfe_dsp_last_error().startswith(b"iir: ") and not h.value


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present: create succeeds there")
def test_create_without_gpu_is_enodev(L):
    from simplefe_amd import api, lib
    with pytest.raises(lib.SfeError) as e:
        api.Iir(synth.iir_dc_blocker(0.995))
    assert e.value.code == lib.SFE_ENODEV


def test_designers():
    assert np.array_equal(synth.iir_dc_blocker(0.25), [[1, -1, 0, 1, -0.25, 0]])
    assert np.array_equal(synth.iir_one_pole(0.25), [[0.75, 0, 0, 1, -0.25, 0]])
    f = np.array([0.0, 0.01, 0.1, 0.125, 0.2, 0.4, 0.5])
    z = np.exp(-2j * np.pi * f)

    def mag(sos):
        h = np.ones_like(z)
        for b0, b1, b2, a0, a1, a2 in sos:
            h = h * (b0 + b1 * z + b2 * z * z) / (a0 + a1 * z + a2 * z * z)
        return np.abs(h)

    assert mag(synth.iir_notch(0.125, 30))[3] < 1e-12 and abs(mag(synth.iir_notch(0.125, 30))[0] - 1) < 1e-12
    for order, fc in ((4, 0.025), (16, 0.1)):
        sos = synth.iir_butter_lowpass(order, fc)
        assert sos.shape == (order // 2, 6)
        want = 1.0 / np.sqrt(1.0 + (np.tan(np.pi * f[:-1]) / np.tan(np.pi * fc)) ** (2 * order))    # the bilinear Butterworth
        assert np.abs(mag(sos)[:-1] - want).max() < 1e-9, (order, fc)
        assert mag(sos)[-1] < 1e-12
    c = synth.iir_round([[2, 1, 0.5, 4, 0.2, 0.1]])
    assert c.dtype == np.float32 and np.array_equal(c, np.array([[0.5, 0.25, 0.125, 0.05, 0.025]], np.float32))


def test_reference_one_pole_impulse_is_the_closed_form():
    (b0, _, _, a1, _), = synth.iir_round(synth.iir_one_pole(0.999)).astype(np.float64)
    x = np.zeros(5000)
    x[0] = 1.0
    y = synth.iir_reference(x, synth.iir_one_pole(0.999))
    want = b0 * (-a1) ** np.arange(5000)
    assert abs(b0 - 0.001) < 1e-10 and abs(-a1 - 0.999) < 1e-7
    assert np.abs(y - want).max() <= 1e-12
    # the float32 form has the law's shape too (first sample exact: one product)
    y32 = synth.iir_reference(x, synth.iir_one_pole(0.999), np.float32)
    assert y32[0] == b0 and np.abs(y32 - want).max() <= 1e-7 * b0 * 5000


def test_reference_agrees_with_scipy_and_with_its_own_loop():
    sig = pytest.importorskip("scipy.signal")
    x = synth.synth_cf32(3000).view(np.complex64)
    for name, sos in FILTERS.items():
        c = synth.iir_round(sos).astype(np.float64)
        rows = np.ascontiguousarray(np.concatenate([c[:, :3], np.ones((len(c), 1)), c[:, 3:]], axis=1))
        want = sig.sosfilt(rows, x.astype(np.complex128))
        got = synth.iir_reference(x, sos)
        loop = synth._iir_loop(np.ascontiguousarray(x.astype(np.complex128)).view(np.float64).reshape(-1, 2), c, np.float64)
        rms = np.sqrt(np.mean(np.abs(want) ** 2))
        assert got.shape == x.shape and np.abs(got - want).max() <= 1e-12 * rms, name
        assert np.abs(loop.view(np.complex128)[:, 0] - want).max() <= 1e-11 * rms, name
    # several streams at once, real and complex
    xs = np.stack([x, x[::-1]])
    ys = synth.iir_reference(xs, FILTERS["butter(4,0.025)"])
    assert np.allclose(ys[1], synth.iir_reference(x[::-1], FILTERS["butter(4,0.025)"]), rtol=0, atol=1e-14)
    yr = synth.iir_reference(x.real, FILTERS["butter(4,0.025)"])
    assert yr.dtype == np.float64 and np.allclose(yr, ys[0].real, rtol=0, atol=1e-14)


def _e32(x, sos):
    r64 = synth.iir_reference(x, sos)
    r32 = synth.iir_reference(x, sos, np.float32)
    return np.sqrt(np.mean(np.abs(r32 - r64) ** 2)) / np.sqrt(np.mean(np.abs(r64) ** 2))


@pytest.mark.parametrize("name", list(FILTERS))
def test_the_yardstick_is_capped_on_the_grid(name):
    """The GPU bars are multiples of the float32 recursion's own error: a careless yardstick must not widen them."""
    e = _e32(synth.synth_cf32(3 * 8192).view(np.complex64), FILTERS[name])
    print("iir yardstick %s: e32 %.2e (cap 1e-5)" % (name, e))
    assert e <= 1e-5, (name, e)


@pytest.mark.parametrize("name", ["dc(0.9999)", "dc(0.995)", "dc(0.999)+butter(8,0.1)"])
def test_the_yardstick_is_capped_on_the_offset_case(name):
    n = 3 * 8192
    x = synth.u8_to_cf32(synth.offset_bytes(n)) + np.complex64(0.3 + 0.2j)
    assert abs(np.mean(x) - (0.3 + 0.2j)) < 0.02
    e = _e32(x, FILTERS[name])
    b = synth.u8_to_cf32(synth.offset_bytes(n, bias=38))
    assert abs(np.mean(synth.offset_bytes(n, bias=38)) - 166) < 1.0 and abs(np.mean(b.real) - 0.3) < 0.01
    eb = _e32(b, FILTERS[name])
    print("iir yardstick, offset %s: e32 %.2e cf32, %.2e bytes (cap 3e-5)" % (name, e, eb))
    assert e <= 3e-5 and eb <= 3e-5, (name, e, eb)


def test_iir_kernels_use_no_scratch():
    from simplefe_amd import build
    build.build_lib()
    res = json.load(open(os.path.join(build.HERE, "build", "iir.hip.resources.json")))
    blocks = {tuple(a.strip() for a in re.search(r"iir_block_kernel<(.*?)>", k).group(1).split(",")) for k in res if "iir_block_kernel<" in k}
    assert blocks == {(str(f), p) for f in range(3) for p in ("false", "true")}
    assert sum("iir_group_kernel<" in k for k in res) == 2 and sum("iir_chain_kernel" in k for k in res) == 1
    for k, v in res.items():
        assert v.get("ScratchSize", 1) == 0 and v.get("VGPRs Spill", 0) == 0 and v.get("SGPRs Spill", 0) == 0, (k, v)


def test_iir_sources_are_in_the_build_lists():
    from simplefe_amd import build
    assert "iir.hip" in build.EXACT_SOURCES and "api_iir.hip" in build.HOST_SOURCES
    assert build.KERNEL_FILES["iir"] == ("iir.hip", "iir.h", "common.h")
    cm = open(os.path.join(ROOT, "CMakeLists.txt")).read()
    assert re.search(r"set\(SFE_EXACT_SOURCES [^)]*\biir\.hip\b", cm)
