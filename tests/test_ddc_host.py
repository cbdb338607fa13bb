"""The digital down-converter bank (sfe_dsp_ddc_*) without a GPU: the C ABI's declarations and exports, the host-only
planner and its frequency quantisation, the no-GPU refusal, the numpy yardsticks the GPU tests compare against, the
kernels' register budget, and the CMake build's contraction-off list."""
import json
import os
import re

import numpy as np
import pytest

from simplefe_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "sfe_dsp.h")
DDC_FUNCS = ("sfe_dsp_ddc_plan", "sfe_dsp_ddc_create", "sfe_dsp_ddc_set_input_format", "sfe_dsp_ddc_set_freqs",
             "sfe_dsp_ddc_process_stream", "sfe_dsp_ddc_reset", "sfe_dsp_ddc_destroy")


@pytest.fixture(scope="module")
def L():
    from simplefe_amd import lib
    return lib.load()


def test_header_declares_ddc_abi_and_library_exports_it(L):
    from simplefe_amd import lib
    declared = set(re.findall(r"\b(sfe_dsp_ddc_[a-z0-9_]+)\s*\(", open(HDR).read()))
    assert declared == set(DDC_FUNCS)
    for name in DDC_FUNCS:
        assert hasattr(L, name), name
        assert name in lib.SIGNATURES, name


@pytest.mark.parametrize("D", [1, 3, 8, 10, 64, 100, 500, 1000, 1024])
def test_plan_accepts_the_supported_shapes(L, D):
    from simplefe_amd import api
    for n_taps in sorted({1, D - 1 or 1, D, D + 1, 8 * D - 3, 16 * D, min(64 * D, 8192)}):
        if -(-n_taps // D) > 64 or n_taps > 8192:
            continue
        for K in (1, 3, 8, 64):
            P, H, incs = api.ddc_plan(n_taps, D, np.linspace(-0.5, 0.5, K))
            assert P == -(-n_taps // D), (D, n_taps, K)
            assert H >= n_taps - 1 and H % D == 0 and H >= P * D, (D, n_taps, H)
            assert incs == synth.ddc_incs(np.linspace(-0.5, 0.5, K))


def test_plan_quantises_the_frequencies(L):
    from simplefe_amd import api
    _, _, incs = api.ddc_plan(64, 8, [0.25, -0.25, 0.5, -0.5, 0.0, 1.0 / 3.0, -1e-9])
    assert incs[:5] == [1 << 30, 3 << 30, 1 << 31, 1 << 31, 0]
    assert incs[5] == round(2 ** 32 / 3) and incs[6] == (1 << 32) - 4
    assert incs == synth.ddc_incs([0.25, -0.25, 0.5, -0.5, 0.0, 1.0 / 3.0, -1e-9])


@pytest.mark.parametrize("n_taps, D, freqs", [(64, 0, [0.1]), (64, 1025, [0.1]), (0, 8, [0.1]), (8193, 1024, [0.1]),
                                              (65 * 8 - 7, 8, [0.1]), (64, 8, []), (64, 8, [0.0] * 65),
                                              (64, 8, [0.1, 0.5000001]), (64, 8, [-0.75]), (64, 8, [float("nan")])])
def test_plan_refuses_other_shapes_with_a_message(L, n_taps, D, freqs):
    from simplefe_amd import api, lib
    with pytest.raises(lib.SfeError) as e:
        api.ddc_plan(n_taps, D, freqs)
    assert e.value.code == lib.SFE_EINVAL
    assert L.sfe_dsp_last_error().startswith(b"ddc: ")


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present: create succeeds there")
def test_create_without_gpu_is_enodev(L):
    from simplefe_amd import api, lib
    with pytest.raises(lib.SfeError) as e:
        api.Ddc(synth.lowpass_taps(64, 1 / 16), 8, [0.1, -0.2])
    assert e.value.code == lib.SFE_ENODEV


def _quadruple_loop(x, h, D, incs):
    y = np.zeros((len(incs), len(x) // D), dtype=np.complex128)
    for k, inc in enumerate(incs):
        for m in range(len(x) // D):
            for n in range(len(h)):
                i = m * D - n
                if i >= 0:
                    y[k, m] += h[n] * x[i] * np.exp(-2j * np.pi * ((i * inc) % (1 << 32)) / 2.0 ** 32)
    return y


@pytest.mark.parametrize("D", [1, 3, 8])
def test_references_equal_the_contract_as_a_quadruple_loop(D):
    rng = np.random.default_rng(D)
    x = rng.standard_normal(72) + 1j * rng.standard_normal(72)
    h = rng.standard_normal(11)
    incs = synth.ddc_incs([0.0, 0.25, -0.5, 0.5, 0.123456789, -0.3])
    want = _quadruple_loop(x, h, D, incs)
    scale = np.abs(want).max()
    n_out = 72 // D
    assert np.abs(synth.ddc_reference(x, h, D, incs) - want).max() <= 1e-12 * scale
    assert np.abs(synth.ddc_reference_direct(x, h, D, incs, 0, 0, n_out) - want).max() <= 1e-12 * scale
    # a window that starts inside the stream, its L-1 preceding samples included
    first = 5 * D - 10 if 5 * D >= 10 else 0
    m0 = 5 if 5 * D >= 10 else 10
    assert np.abs(synth.ddc_reference_direct(x[first:], h, D, incs, first, m0, n_out - m0) - want[:, m0:]).max() <= 1e-12 * scale
    # the phase is the absolute sample index's: a stream that starts later is another stream
    assert np.abs(synth.ddc_reference(x[2 * D:], h, D, incs, first=2 * D)[:, 3:] - want[:, 5:]).max() > 0


def test_rotated_taps_equal_the_mixed_data():
    """The kernel's identity: y_k[m] = exp(-j 2 pi phi_k(mD)) sum_n g_k[n] x[mD - n], g_k[n] = h[n] exp(+j 2 pi phi_k(n))."""
    rng = np.random.default_rng(7)
    D, L, n = 10, 37, 400
    x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    h = rng.standard_normal(L)
    incs = synth.ddc_incs([0.5, -0.5, 0.1, -0.37])
    want = synth.ddc_reference(x, h, D, incs)
    for k, inc in enumerate(incs):
        g = h * np.conj(synth._ddc_phase(np.arange(L), inc))
        m = np.arange(n // D)
        full = np.convolve(x, g)[: n][m * D]
        got = synth._ddc_phase(m * D, inc) * full
        assert np.abs(got - want[k]).max() <= 5e-15 * np.abs(want[k]).max() * L


def test_ddc_kernels_use_no_scratch():
    from simplefe_amd import build
    build.build_lib()
    res = json.load(open(os.path.join(build.HERE, "build", "ddc.hip.resources.json")))
    kernels = {k: v for k, v in res.items() if "ddc_kernel<" in k}
    shapes = {tuple(a.strip() for a in re.search(r"ddc_kernel<(.*?)>", k).group(1).split(",")) for k in kernels}
    assert {(f, kt) for f, kt, _, _ in shapes} == {(str(f), str(kt)) for f in range(3) for kt in (1, 2, 4, 8)}
    assert {s[3] for s in shapes} == {"false", "true"}
    assert len(shapes) == 24
    for k, v in res.items():
        assert v.get("ScratchSize", 1) == 0 and v.get("VGPRs Spill", 0) == 0 and v.get("SGPRs Spill", 0) == 0, (k, v)


def test_cmake_contraction_off_list_equals_build_py():
    from simplefe_amd import build
    text = open(os.path.join(ROOT, "CMakeLists.txt")).read()
    m = re.search(r"set\(SFE_EXACT_SOURCES([^)]*)\)", text)
    assert m, "CMakeLists.txt names the sources it compiles with -ffp-contract=off in SFE_EXACT_SOURCES"
    assert set(m.group(1).split()) == set(build.EXACT_SOURCES)
    assert "ddc.hip" in build.EXACT_SOURCES and "chan.hip" in build.EXACT_SOURCES
    # and that list is the one the flag follows
    assert re.search(r"if\(name IN_LIST SFE_EXACT_SOURCES\)\s*\n\s*list\(APPEND flags -ffp-contract=off\)", text)
