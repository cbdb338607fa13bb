"""The streaming preamble correlator bank (sfe_dsp_corr_*) without a GPU: the C ABI's declarations and exports, the
host-only planner, the refusals that precede the device, the numpy yardsticks the GPU tests compare against, and the
kernels' register budget."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from simplefe_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "sfe_dsp.h")
# the functions of the C ABI
CORR_FUNCS = ("sfe_dsp_corr_plan", "sfe_dsp_corr_create", "sfe_dsp_corr_set_input_format", "sfe_dsp_corr_process_stream",
              "sfe_dsp_corr_reset", "sfe_dsp_corr_destroy")


@pytest.fixture(scope="module")
def L():
    from simplefe_amd import lib
    return lib.load()


def test_header_declares_corr_abi_and_library_exports_it(L):
    from simplefe_amd import lib
    text = open(HDR).read()
    declared = set(re.findall(r"\b(sfe_dsp_corr_[a-z0-9_]+)\s*\(", text))
    assert declared == set(CORR_FUNCS)
    assert re.search(r"typedef\s+void\s*\*\s*sfe_corr_t\s*;", text)
    for name in CORR_FUNCS:
        assert hasattr(L, name), name
        assert name in lib.SIGNATURES, name


@pytest.mark.parametrize("length, advance, history", [(1, 4096, 0), (13, 3840, 256), (256, 3840, 256), (257, 3840, 256),
                                                      (258, 3584, 512), (2049, 2048, 2048)])
def test_plan_reports_advance_and_history(L, length, advance, history):
    from simplefe_amd import api
    assert api.corr_plan(length, 3, 2 * advance) == (advance, history)
    # sfe_dsp_fir_plan's rule for a single partition
    assert advance == 4096 - 256 * -(-(length - 1) // 256)


@pytest.mark.parametrize("length, K, B", [(0, 1, 4096), (2050, 1, 2048), (13, 0, 3840), (13, 17, 3840), (13, 1, 0), (13, 1, 3841),
                                          (13, 1, 4096), (13, 1, -3840)])
def test_plan_refuses_other_shapes_with_a_message(L, length, K, B):
    from simplefe_amd import api, lib
    with pytest.raises(lib.SfeError) as e:
        api.corr_plan(length, K, B)
    assert e.value.code == lib.SFE_EINVAL
    assert L.sfe_dsp_last_error().startswith(b"corr: ")


def _create(L, templates, block, min_energy):
    t = np.ascontiguousarray(templates, dtype=np.complex64)
    h = C.c_void_p()
    rc = L.sfe_dsp_corr_create(t.view(np.float32).ctypes.data, t.shape[1], t.shape[0], block, min_energy, 1, 0, C.byref(h))
    if h.value:
        L.sfe_dsp_corr_destroy(h)
    return rc


@pytest.mark.parametrize("min_energy", [-1e-6, float("inf"), float("nan")])
def test_create_refuses_a_bad_gate_before_it_looks_for_a_device(L, min_energy):
    from simplefe_amd import lib
    t = synth.synth_cf32(2 * 13).view(np.complex64).reshape(2, 13)
    assert _create(L, t, 3840, min_energy) == lib.SFE_EINVAL
    assert L.sfe_dsp_last_error().startswith(b"corr: ")


def test_create_refuses_an_all_zero_template_before_it_looks_for_a_device(L):
    from simplefe_amd import lib
    t = synth.synth_cf32(3 * 13).view(np.complex64).reshape(3, 13).copy()
    t[1] = 0
    assert _create(L, t, 3840, 1e-6) == lib.SFE_EINVAL
    assert L.sfe_dsp_last_error().startswith(b"corr: ")
    t[1, 0] = np.nan
    assert _create(L, t, 3840, 1e-6) == lib.SFE_EINVAL


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present: create succeeds there")
def test_create_without_gpu_is_enodev(L):
    from simplefe_amd import api, lib
    with pytest.raises(lib.SfeError) as e:
        api.Corr(synth.synth_cf32(13).view(np.complex64), 3840, 1e-6)
    assert e.value.code == lib.SFE_ENODEV


def test_references_agree():
    Lt, K, B, gate = 37, 3, 256, 1e-6
    t = synth.synth_cf32(K * Lt, ch=5).view(np.complex64).reshape(K, Lt)
    x = synth.synth_cf32(6 * B).view(np.complex64).copy()
    x[700:700 + Lt] += t[1]
    x[900:1100] = 0                         # windows the gate shuts
    m, pv, pi = synth.corr_reference(x, t, B, gate)
    assert m.shape == (K, 6 * B) and pv.shape == pi.shape == (K, 6)
    # the window reaches before the stream (i < L - 1), lies in it, ends on the planted template, is gated
    points = [(0, 0), (1, 5), (2, Lt - 2), (0, Lt - 1), (1, 700 + Lt - 1), (2, 700 + Lt - 1), (1, 699 + Lt), (0, 1000), (2, 1098),
              (0, 1099 + Lt), (1, 6 * B - 1), (2, 3 * B)]
    d = synth.corr_reference_direct(x, t, gate, 0, points)
    assert np.abs(d - np.array([m[k, i] for k, i in points])).max() <= 1e-12
    assert d[7] == 0.0 and m[0, 1000] == 0.0 and d[4] > 0.3      # planted at the noise's own power: about one half
    assert pi[1, 700 // B + (700 % B + Lt - 1) // B] == (700 + Lt - 1) % B
    # a stream taken up later: the L - 1 samples before `first` lead it
    first = 2 * B
    late, lv, li = synth.corr_reference(x[first - (Lt - 1):], t, B, gate, first=first)
    assert late.shape == (K, 4 * B)
    assert np.abs(late - m[:, first:]).max() <= 1e-12
    assert np.array_equal(li, pi[:, 2:]) and np.abs(lv - pv[:, 2:]).max() <= 1e-12
    later = [(k, i) for k, i in points if i >= first + Lt] + [(0, first), (2, first + 3)]
    d2 = synth.corr_reference_direct(x[first - (Lt - 1):], t, gate, first - (Lt - 1), later)
    assert np.abs(d2 - np.array([m[k, i] for k, i in later])).max() <= 1e-12
    # and through the transforms the reference takes for long templates
    t2 = synth.synth_cf32(2 * 300, ch=6).view(np.complex64).reshape(2, 300)
    m2, _, _ = synth.corr_reference(x, t2, B, gate)
    pts = [(0, 3), (1, 299), (0, 1200), (1, 6 * B - 1)]
    assert np.abs(synth.corr_reference_direct(x, t2, gate, 0, pts) - np.array([m2[k, i] for k, i in pts])).max() <= 1e-12


def test_a_window_that_is_a_multiple_of_the_template_gives_one():
    Lt, B = 29, 128
    t = synth.synth_cf32(2 * Lt, ch=9).view(np.complex64).reshape(2, Lt)
    x = synth.synth_cf32(4 * B).view(np.complex64).copy()
    x[200:200 + Lt] = 0.3 * t[1]
    m, pv, pi = synth.corr_reference(x, t, B, 1e-6)
    i = 200 + Lt - 1
    assert abs(m[1, i] - 1.0) <= 1e-12
    assert pi[1, i // B] == i % B and abs(pv[1, i // B] - 1.0) <= 1e-12
    assert abs(synth.corr_reference_direct(x, t, 1e-6, 0, [(1, i)])[0] - 1.0) <= 1e-12
    assert m[0, i] < 0.5 and m.max() <= 1.0 + 1e-12


def test_corr_kernels_use_no_scratch():
    from simplefe_amd import build
    build.build_lib()
    res = json.load(open(os.path.join(build.HERE, "build", "corr.hip.resources.json")))
    slot = {tuple(a.strip() for a in re.search(r"corr_slot_kernel<(.*?)>", k).group(1).split(",")) for k in res if "corr_slot_kernel<" in k}
    tf = ("false", "true")
    assert slot == {(u8, dense, direct) for u8 in tf for dense in tf for direct in tf}
    assert sum("corr_fold_kernel" in k for k in res) == 1 and sum("corr_hist_kernel<" in k for k in res) == 2
    for k, v in res.items():
        assert v.get("ScratchSize", 1) == 0 and v.get("VGPRs Spill", 0) == 0 and v.get("SGPRs Spill", 0) == 0, (k, v)
        if "corr_slot_kernel<" in k:        # two workgroups per CU at the least: 256 threads, so 256 registers per thread
            assert v["VGPRs"] <= 256 and v["LDS Size"] <= 80 * 1024, (k, v)


def test_corr_sources_are_in_the_build_lists():
    from simplefe_amd import build
    assert "corr.hip" in build.EXACT_SOURCES and "api_corr.hip" in build.HOST_SOURCES
    assert build.KERNEL_FILES["corr"] == ("corr.hip", "fft16.h", "common.h")
    cm = open(os.path.join(ROOT, "CMakeLists.txt")).read()
    assert re.search(r"SFE_EXACT_SOURCES[^)]*\bcorr\.hip", cm)
