"""The polyphase channelizer (sfe_dsp_chan_*) without a GPU: the C ABI's declarations and exports, the host-only shape
planner, the no-GPU refusal, the numpy yardstick the GPU tests compare against, and the kernels' register budget."""
import json
import os
import re

import numpy as np
import pytest

from simplefe_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "sfe_dsp.h")
CHAN_FUNCS = ("sfe_dsp_chan_plan", "sfe_dsp_chan_create", "sfe_dsp_chan_set_input_format", "sfe_dsp_chan_process_stream",
              "sfe_dsp_chan_reset", "sfe_dsp_chan_destroy")


@pytest.fixture(scope="module")
def L():
    from simplefe_amd import lib
    return lib.load()


def test_header_declares_chan_abi_and_library_exports_it(L):
    from simplefe_amd import lib
    declared = set(re.findall(r"\b(sfe_dsp_chan_[a-z0-9_]+)\s*\(", open(HDR).read()))
    assert declared == set(CHAN_FUNCS)
    for name in CHAN_FUNCS:
        assert hasattr(L, name), name
        assert name in lib.SIGNATURES, name


@pytest.mark.parametrize("M", [4, 8, 16, 64, 256, 512, 1024])
def test_plan_accepts_the_supported_shapes(L, M):
    from simplefe_amd import api
    for D in (M, M // 2):
        for n_taps in (1, M - 1, M, M + 1, 8 * M - 3, 16 * M, 32 * M):
            P, H = api.chan_plan(n_taps, M, D)
            assert P == -(-n_taps // M), (M, D, n_taps)
            assert H >= n_taps - 1 and H % M == 0, (M, D, n_taps, H)


@pytest.mark.parametrize("n_taps, M, D", [(16, 2, 2), (16, 2, 1), (16, 3, 3), (16, 2048, 2048), (64, 64, 16),
                                          (64, 64, 3), (0, 64, 64), (32 * 64 + 1, 64, 64), (32 * 64 + 1, 64, 32)])
def test_plan_refuses_other_shapes_with_a_message(L, n_taps, M, D):
    from simplefe_amd import api, lib
    with pytest.raises(lib.SfeError) as e:
        api.chan_plan(n_taps, M, D)
    assert e.value.code == lib.SFE_EINVAL
    assert L.sfe_dsp_last_error().startswith(b"chan: ")


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present: create succeeds there")
def test_create_without_gpu_is_enodev(L):
    from simplefe_amd import api, lib
    with pytest.raises(lib.SfeError) as e:
        api.Chan(synth.lowpass_taps(64, 1 / 16), 16, 16)
    assert e.value.code == lib.SFE_ENODEV


def _triple_loop(x, h, M, D):
    y = np.zeros((M, len(x) // D), dtype=np.complex128)
    for k in range(M):
        for m in range(len(x) // D):
            for n in range(len(h)):
                i = m * D - n
                if i >= 0:
                    y[k, m] += h[n] * x[i] * np.exp(-2j * np.pi * k * i / M)
    return y


@pytest.mark.parametrize("M", [4, 8])
def test_reference_equals_the_contract_as_a_triple_loop(M):
    rng = np.random.default_rng(M)
    x = rng.standard_normal(64) + 1j * rng.standard_normal(64)
    h = rng.standard_normal(11)
    for D in (M, M // 2):
        want = _triple_loop(x, h, M, D)
        scale = np.abs(want).max()
        assert np.abs(synth.chan_reference(x, h, M, D) - want).max() <= 1e-12 * scale
        assert np.abs(synth.chan_reference_direct(x, h, M, D, 0, 0, 64 // D) - want).max() <= 1e-12 * scale
        # a window that starts inside the stream, its L-1 preceding samples included
        first = 5 * D - 10
        assert np.abs(synth.chan_reference_direct(x[first:], h, M, D, first, 5, 64 // D - 5) - want[:, 5:]).max() <= 1e-12 * scale
        assert np.abs(synth.chan_reference(x[2 * D:], h, M, D, first=2 * D)[:, 3:] - want[:, 5:]).max() > 0   # no history there


def test_chan_kernels_use_no_scratch():
    from simplefe_amd import build
    build.build_lib()
    res = json.load(open(os.path.join(build.HERE, "build", "chan.hip.resources.json")))
    kernels = {k: v for k, v in res.items() if "chan_kernel<" in k}
    shapes = {tuple(a.strip() for a in re.search(r"chan_kernel<(.*?)>", k).group(1).split(",")) for k in kernels}
    assert shapes == {(str(lm), d, f) for lm in range(2, 11) for d in ("false", "true") for f in ("false", "true")}
    for k, v in res.items():
        assert v.get("ScratchSize", 1) == 0 and v.get("VGPRs Spill", 0) == 0, (k, v)
