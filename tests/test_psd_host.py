"""The streaming Welch spectrum estimator (sfe_dsp_psd_*) without a GPU: the C ABI's declarations and exports, the
host-only planner, the no-GPU refusal, the numpy yardsticks the GPU tests compare against, and the kernels' register
budget."""
import json
import os
import re

import numpy as np
import pytest

from simplefe_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "sfe_dsp.h")
PSD_FUNCS = ("sfe_dsp_psd_plan", "sfe_dsp_psd_create", "sfe_dsp_psd_set_input_format", "sfe_dsp_psd_process_stream",
             "sfe_dsp_psd_reset", "sfe_dsp_psd_destroy")


@pytest.fixture(scope="module")
def L():
    from simplefe_amd import lib
    return lib.load()


def test_header_declares_psd_abi_and_library_exports_it(L):
    from simplefe_amd import lib
    declared = set(re.findall(r"\b(sfe_dsp_psd_[a-z0-9_]+)\s*\(", open(HDR).read()))
    assert declared == set(PSD_FUNCS)
    for name in PSD_FUNCS:
        assert hasattr(L, name), name
        assert name in lib.SIGNATURES, name


@pytest.mark.parametrize("N, H, A, chunk, history", [(256, 256, 1, 1, 0), (1024, 384, 37, 8, 640), (4096, 2048, 65536, 256, 2048)])
def test_plan_reports_chunk_and_history(L, N, H, A, chunk, history):
    from simplefe_amd import api
    assert api.psd_plan(N, H, A) == (chunk, history)


@pytest.mark.parametrize("A", [1, 2, 3, 4, 5, 16, 17, 37, 64, 65, 4096, 4097, 1 << 24])
def test_chunk_is_the_smallest_power_of_two_whose_square_reaches_n_avg(L, A):
    from simplefe_amd import api
    c, _ = api.psd_plan(1024, 512, A)
    assert c & (c - 1) == 0 and c * c >= A and (c == 1 or (c // 2) ** 2 < A)


@pytest.mark.parametrize("N, H, A", [(128, 64, 4), (8192, 4096, 4), (1000, 500, 4), (1024, 0, 4), (1024, 1025, 4), (1024, 512, 0)])
def test_plan_refuses_other_shapes_with_a_message(L, N, H, A):
    from simplefe_amd import api, lib
    with pytest.raises(lib.SfeError) as e:
        api.psd_plan(N, H, A)
    assert e.value.code == lib.SFE_EINVAL
    assert L.sfe_dsp_last_error().startswith(b"psd: ")


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present: create succeeds there")
def test_create_without_gpu_is_enodev(L):
    from simplefe_amd import api, lib
    with pytest.raises(lib.SfeError) as e:
        api.Psd(np.hanning(1024), 512, 8)
    assert e.value.code == lib.SFE_ENODEV


def test_references_agree():
    N, H, A = 256, 96, 5
    first = 777
    w = np.hanning(N)
    x = synth.synth_cf32(first + 3 * A * H + 3 * N).view(np.complex64)
    bins = [0, 1, N // 2, N - 1]
    whole = synth.psd_reference(x, w, H, A, 0.25)
    r_lo, r_hi = synth.psd_rows(x.size - first, N, H, A, first)
    assert r_lo > 0 and r_hi - r_lo >= 3 and r_hi == whole.shape[0]
    late = synth.psd_reference(x[first:], w, H, A, 0.25, first=first)
    assert late.shape == (r_hi - r_lo, N)
    for r in range(r_lo, r_lo + 3):
        peak = np.abs(whole[r]).max()
        d = synth.psd_reference_direct(x[first:], w, H, A, 0.25, first, r, bins)
        assert np.abs(d - whole[r][bins]).max() <= 1e-12 * peak, r
        assert np.abs(late[r - r_lo] - whole[r]).max() <= 1e-12 * peak, r
    # row 0 reaches before the stream: zeros there
    d0 = synth.psd_reference_direct(x, w, H, A, 0.25, 0, 0, bins)
    assert np.abs(d0 - whole[0][bins]).max() <= 1e-12 * np.abs(whole[0]).max()


@pytest.mark.parametrize("k0", [3, 253])
def test_an_on_bin_tone_under_a_rectangular_window(k0):
    N, H, A, a, scale = 256, 128, 6, 0.375, 0.5
    x = a * np.exp(2j * np.pi * k0 * np.arange(H * (3 * A)) / N)
    rows = synth.psd_reference(x, np.ones(N), H, A, scale)
    want = scale * A * (a * N) ** 2
    for r in (1, 2):                        # row 0 has the segments that reach before the stream
        assert int(np.argmax(rows[r])) == k0
        assert abs(rows[r][k0] - want) <= 1e-12 * want
        assert np.delete(rows[r], k0).max() <= 1e-20 * want
    got = synth.psd_reference_direct(x, np.ones(N), H, A, scale, 0, 1, [k0])[0]
    assert abs(got - want) <= 1e-12 * want


def test_psd_kernels_use_no_scratch():
    from simplefe_amd import build
    build.build_lib()
    res = json.load(open(os.path.join(build.HERE, "build", "psd.hip.resources.json")))
    chunk = {tuple(a.strip() for a in re.search(r"psd_chunk_kernel<(.*?)>", k).group(1).split(",")) for k in res if "psd_chunk_kernel<" in k}
    assert chunk == {(str(lg), u8) for lg in range(8, 13) for u8 in ("false", "true")}
    assert sum("psd_row_kernel<" in k for k in res) == 5 and sum("psd_hist_kernel<" in k for k in res) == 2
    for k, v in res.items():
        assert v.get("ScratchSize", 1) == 0 and v.get("VGPRs Spill", 0) == 0 and v.get("SGPRs Spill", 0) == 0, (k, v)


def test_psd_sources_are_in_the_build_lists():
    from simplefe_amd import build
    assert "psd.hip" in build.EXACT_SOURCES and "api_psd.hip" in build.HOST_SOURCES
    assert build.KERNEL_FILES["psd"] == ("psd.hip", "fft16.h", "common.h")
