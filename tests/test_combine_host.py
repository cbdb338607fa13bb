"""The polyphase synthesis filter bank (sfe_dsp_combine_*) without a GPU: the C ABI's declarations and exports, the
host-only shape planner, the no-GPU refusal, the numpy yardsticks the GPU tests compare against, the channelizer ->
combiner round trip in float64, and the kernels' register budget."""
import json
import os
import re

import numpy as np
import pytest

from simplefe_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "sfe_dsp.h")
COMBINE_FUNCS = ("sfe_dsp_combine_plan", "sfe_dsp_combine_create", "sfe_dsp_combine_set_output_format",
                 "sfe_dsp_combine_process_stream", "sfe_dsp_combine_reset", "sfe_dsp_combine_destroy")


@pytest.fixture(scope="module")
def L():
    from simplefe_amd import lib
    return lib.load()


def test_header_declares_combine_abi_and_library_exports_it(L):
    from simplefe_amd import lib
    declared = set(re.findall(r"\b(sfe_dsp_combine_[a-z0-9_]+)\s*\(", open(HDR).read()))
    assert declared == set(COMBINE_FUNCS)
    for name in COMBINE_FUNCS:
        assert hasattr(L, name), name
        assert name in lib.SIGNATURES, name


@pytest.mark.parametrize("M", [4, 8, 16, 64, 256, 512, 1024])
def test_plan_accepts_the_supported_shapes(L, M):
    from simplefe_amd import api
    for D in (M, M // 2):
        for n_taps in (1, M - 1, M, M + 1, 8 * M - 3, 16 * M, 32 * M):
            P, H = api.combine_plan(n_taps, M, D)
            assert P == -(-n_taps // D), (M, D, n_taps)
            assert H >= P - 1, (M, D, n_taps, H)


@pytest.mark.parametrize("n_taps, M, D", [(16, 2, 2), (16, 2, 1), (16, 3, 3), (16, 2048, 2048), (64, 64, 16),
                                          (64, 64, 3), (64, 64, 128), (0, 64, 64), (32 * 64 + 1, 64, 64),
                                          (32 * 64 + 1, 64, 32)])
def test_plan_refuses_other_shapes_with_a_message(L, n_taps, M, D):
    from simplefe_amd import api, lib
    with pytest.raises(lib.SfeError) as e:
        api.combine_plan(n_taps, M, D)
    assert e.value.code == lib.SFE_EINVAL
    assert L.sfe_dsp_last_error().startswith(b"combine: ")


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present: create succeeds there")
def test_create_without_gpu_is_enodev(L):
    from simplefe_amd import api, lib
    with pytest.raises(lib.SfeError) as e:
        api.Combiner(synth.lowpass_taps(64, 1 / 16), 16, 16)
    assert e.value.code == lib.SFE_ENODEV


def _triple_loop(X, g, M, D):
    n = X.shape[1]
    z = np.zeros(n * D, dtype=np.complex128)
    for i in range(n * D):
        for m in range(n):
            t = i - m * D
            if 0 <= t < len(g):
                for k in range(M):
                    z[i] += g[t] * X[k, m] * np.exp(2j * np.pi * k * i / M)
    return z


@pytest.mark.parametrize("M", [4, 8])
def test_references_equal_the_contract_as_a_triple_loop(M):
    rng = np.random.default_rng(M)
    n = 12
    X = rng.standard_normal((M, n)) + 1j * rng.standard_normal((M, n))
    g = rng.standard_normal(3 * M + 1)
    for D in (M, M // 2):
        want = _triple_loop(X, g, M, D)
        scale = np.abs(want).max()
        assert np.abs(synth.combine_reference(X, g, M, D) - want).max() <= 1e-12 * scale
        assert np.abs(synth.combine_reference_direct(X, g, M, D, 0, 0, n * D) - want).max() <= 1e-12 * scale
        # a window inside the stream, from the instants it reaches only
        i0 = 7 * D + 3
        first = -(-(i0 - g.size + 1) // D)
        got = synth.combine_reference_direct(X[:, first:], g, M, D, first, i0, n * D - i0)
        assert np.abs(got - want[i0:]).max() <= 1e-12 * scale
        # the overlap-add form with `first`: instants before it are zero, so only its own outputs' tails differ
        tail = synth.combine_reference(X[:, 5:], g, M, D, first=5)
        ref5 = _triple_loop(np.concatenate([np.zeros((M, 5)), X[:, 5:]], axis=1), g, M, D)[5 * D:]
        assert np.abs(tail - ref5).max() <= 1e-12 * scale


def _round_trip(M, n_h):
    """x -> channelizer (D = M/2, h = lowpass(n_h, 2/M)) -> combiner (D = M/2, g = lowpass(n_h, 1/M)), float64;
    returns (relative error against the best complex gain times x delayed by (n_h - 1) samples, that gain)."""
    D = M // 2
    h = synth.lowpass_taps(n_h, 2.0 / M).astype(np.float64)
    g = synth.lowpass_taps(n_h, 1.0 / M).astype(np.float64)
    rng = np.random.default_rng(M)
    n = 160 * M
    x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    Y = synth.chan_reference(x, h, M, D)                              # (M, n / D)
    z = synth.combine_reference(Y, g, M, D)
    delay = n_h - 1
    lo = 2 * delay
    a, b = z[lo:], x[lo - delay:n - delay]
    gain = np.vdot(b, a) / np.vdot(b, b)
    err = np.sqrt(np.mean(np.abs(a - gain * b) ** 2)) / np.sqrt(np.mean(np.abs(gain * b) ** 2))
    return err, gain


@pytest.mark.parametrize("M", [16, 64])
def test_channelizer_then_combiner_gives_the_input_back(M):
    err, gain = _round_trip(M, 16 * M + 1)
    assert err <= 2.5e-3, (M, err)
    assert abs(gain - 2.0 / M) <= 0.01 * (2.0 / M), (M, gain)


def test_combine_kernels_use_no_scratch():
    from simplefe_amd import build
    build.build_lib()
    res = json.load(open(os.path.join(build.HERE, "build", "combine.hip.resources.json")))
    kernels = {k: v for k, v in res.items() if "combine_kernel<" in k}
    shapes = {tuple(a.strip() for a in re.search(r"combine_kernel<(.*?)>", k).group(1).split(",")) for k in kernels}
    assert shapes == {(str(lm), d, str(lj)) for lm in range(2, 11) for d, ljs in (("false", (3, 4, 5)), ("true", (3, 4, 5, 6)))
                      for lj in ljs}
    assert any("combine_hist_kernel" in k for k in res)
    for k, v in res.items():
        assert v.get("ScratchSize", 1) == 0 and v.get("VGPRs Spill", 0) == 0 and v.get("SGPRs Spill", 0) == 0, (k, v)
