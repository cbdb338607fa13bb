"""The occupancy detector's host plan (sfe_dsp_occ_plan: csrc/occ_law.h compiled for the host) against synth.occ_reference,
the numpy restatement of the law -- np.sort for the floor, explicit float32 folds -- byte for byte: random rows at every
kind of size, and constructed rows of which each hits one branch and is also held to what the law must give there
(tests/occ_cases.py).  Then the plan's refusals, and the same constructed rows through a stand-alone program built with
-fsanitize=address,undefined (tests/host/test_occ_law.cpp).  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import occ_cases as oc
from simplefe_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = oc.constructed()


@pytest.fixture(scope="module")
def api():
    from simplefe_amd import api as a, build
    build.build_lib()
    return a


@pytest.fixture(scope="module")
def L():
    from simplefe_amd import lib
    return lib


def same_bytes(got, want, what):
    for name, g, w in zip(("info", "rec", "mask"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        gb, wb = np.ascontiguousarray(g).view(np.uint8).reshape(g.shape[0], -1), np.ascontiguousarray(w).view(np.uint8).reshape(w.shape[0], -1)
        d = gb != wb
        assert not d.any(), "%s: %s differs in %d bytes, the first in row %d at byte %d: %r != %r" % (
            what, name, int(d.sum()), *np.argwhere(d)[0], g[np.argwhere(d)[0][0]], w[np.argwhere(d)[0][0]])


def test_the_structured_dtypes_are_the_abis(api):
    assert api.OCC_INFO.itemsize == 16 and api.OCC_REC.itemsize == 32
    assert api.OCC_INFO == synth.OCC_INFO and api.OCC_REC == synth.OCC_REC


@pytest.mark.parametrize("N", [8, 16, 250, 256, 1024, 4096])
def test_random_rows_give_the_reference_bytes(api, N):
    rows = oc.random_rows(N, 24 if N <= 1024 else 8, seed=N)
    seen = 0
    for k, base in enumerate(oc.SETS):
        for shift in ((False, True) if N % 2 == 0 else (False,)):
            p = oc.params(N, **dict(base, shift=shift))
            got, want = api.occ_plan(rows, **p), synth.occ_reference(rows, **p)
            same_bytes(got, want, "N %d, set %d, shift %d" % (N, k, shift))
            seen += int(want[0]["count"].sum())
    assert seen > 0                                 # the rows do hold emissions


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_constructed_rows(api, case):
    name, rows, p, check = case
    got = api.occ_plan(rows, **p)
    same_bytes(got, synth.occ_reference(rows, **p), name)
    check(*got)


def test_the_mask_is_in_the_rows_own_numbering_under_shift(api):
    N = 256
    rows = oc.random_rows(N, 8, seed=5)
    p = oc.params(N, rank=0.25, factor=4.0, gap=1, shift=True)
    info, rec, mask = api.occ_plan(rows, **p)
    q = dict(p, shift=False)
    info0, rec0, mask0 = api.occ_plan(np.roll(rows, N // 2, axis=1), **q)         # the scan order laid out as a row
    assert np.array_equal(mask, np.roll(mask0, -N // 2, axis=1)) and mask.any()
    assert np.array_equal(info, info0)
    for f in ("lo", "hi", "peak"):
        live = np.arange(rec.shape[1])[None, :] < np.minimum(info["count"], rec.shape[1])[:, None]
        assert np.array_equal((rec[f] + N // 2)[live], rec0[f][live])
    for f in ("peak_val", "sum", "moment"):
        assert np.array_equal(rec[f].view(np.uint32), rec0[f].view(np.uint32))


def test_outputs_are_optional_and_do_not_change_one_another(api, L):
    N, E = 250, 4
    rows = oc.random_rows(N, 6, seed=11)
    p = oc.params(N, rank=60, factor=3.0, gap=1, max_emissions=E)
    info, rec, mask = api.occ_plan(rows, **p)
    lib = L.load()
    head = (N, p["rank"], p["factor"], p["min_level"], p["gap"], p["min_width"], E, 0, rows.ctypes.data_as(L.fp), rows.shape[0])
    i2, r2, m2 = np.empty_like(info), np.empty_like(rec), np.empty_like(mask)
    assert lib.sfe_dsp_occ_plan(*head, i2.ctypes.data, None, None) == L.SFE_OK and np.array_equal(i2, info)
    assert lib.sfe_dsp_occ_plan(*head, None, r2.ctypes.data, None) == L.SFE_OK and np.array_equal(r2, rec)
    assert lib.sfe_dsp_occ_plan(*head, None, None, m2.ctypes.data) == L.SFE_OK and np.array_equal(m2, mask)
    assert lib.sfe_dsp_occ_plan(*head, None, None, None) == L.SFE_OK


def test_refusals_and_their_prefix(api, L):
    lib = L.load()
    good = dict(n_bins=64, rank=16, factor=2.0, min_level=0.0, gap=2, min_width=1, max_emissions=16, shift=1)
    order = ("n_bins", "rank", "factor", "min_level", "gap", "min_width", "max_emissions", "shift")
    assert lib.sfe_dsp_occ_plan(*[good[k] for k in order], None, 0, None, None, None) == L.SFE_OK
    bad = [("n_bins", 7), ("n_bins", 4097), ("n_bins", 63), ("rank", -1), ("rank", 64), ("factor", 0.0), ("factor", -1.0),
           ("factor", float("inf")), ("factor", float("nan")), ("min_level", float("nan")), ("min_level", float("-inf")),
           ("gap", -1), ("gap", 64), ("min_width", 0), ("min_width", 65), ("max_emissions", 0), ("max_emissions", 65),
           ("shift", 2), ("shift", -1)]
    h = C.c_void_p(1)
    for k, v in bad:
        a = [dict(good, **{k: v})[n] for n in order]
        assert lib.sfe_dsp_occ_plan(*a, None, 0, None, None, None) == L.SFE_EINVAL, (k, v)
        assert lib.sfe_dsp_last_error().startswith(b"occ: "), lib.sfe_dsp_last_error()
        # create refuses them before it looks for a device: SFE_EINVAL on a machine with no GPU too
        assert lib.sfe_dsp_occ_create(*a, 0, C.byref(h)) == L.SFE_EINVAL and h.value is None, (k, v)
        assert lib.sfe_dsp_last_error().startswith(b"occ: ")
        h.value = 1
    odd = [dict(good, n_bins=63, rank=16, shift=0)[n] for n in order]           # an odd N is fine without shift
    assert lib.sfe_dsp_occ_plan(*odd, None, 0, None, None, None) == L.SFE_OK
    assert lib.sfe_dsp_occ_plan(*[good[k] for k in order], None, 3, None, None, None) == L.SFE_EINVAL     # rows missing
    assert lib.sfe_dsp_last_error().startswith(b"occ: ")
    with pytest.raises(api.SfeError):
        api.occ_plan(np.ones((2, 64), np.float32), rank=64, factor=2.0)
    if not os.path.exists("/dev/kfd"):
        with pytest.raises(api.SfeError) as e:
            api.Occ(64, 16, 2.0)
        assert e.value.code == L.SFE_ENODEV
    k = C.c_size_t(5)
    assert lib.sfe_dsp_occ_process_stream(None, None, 1, 1, 64, None, None, None, 1, C.byref(k), None) == L.SFE_EINVAL and k.value == 0
    assert lib.sfe_dsp_last_error().startswith(b"occ_process_stream: ")
    assert lib.sfe_dsp_occ_destroy(None) == L.SFE_OK


def test_the_kernel_is_registered_and_touches_no_scratch(api):
    import json
    import re
    from simplefe_amd import build
    res = json.load(open(os.path.join(build.HERE, "build", "occ.hip.resources.json")))
    assert len(res) == 3 and all("occ_kernel<" in k for k in res)          # one wave to 256 bins, four waves to 1024 and to 4096
    for k, r in res.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (k, r)
        assert r["LDS Size"] <= 24 * 1024 and r["Occupancy"] >= 7, (k, r)
    assert "occ.hip" in build.EXACT_SOURCES and "api_occ.hip" in build.HOST_SOURCES and build.SCRATCH_FREE["occ.hip"]
    assert build.KERNEL_FILES["occ"] == ("occ.hip", "occ.h", "occ_law.h", "common.h")
    cm = open(os.path.join(ROOT, "CMakeLists.txt")).read()
    assert re.search(r"set\(SFE_EXACT_SOURCES [^)]*\bocc\.hip\b", cm)


def test_the_law_under_the_sanitizers(tmp_path):
    """tests/host/test_occ_law.cpp, built with the host compiler and -fsanitize=address,undefined, runs occ_plan_row over the
    constructed rows (and a few random ones) from heap blocks of exactly the contract's sizes; what it writes is the
    reference's, byte for byte."""
    exe, fin, fout = str(tmp_path / "occ_law"), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    r = subprocess.run(["g++", "-O1", "-Wall", "-std=c++14", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests/host/test_occ_law.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    cases = [(n, rows, p) for n, rows, p, _ in CASES]
    for N in (8, 250, 4096):
        for k, base in enumerate(oc.SETS):
            cases.append(("random N %d set %d" % (N, k), oc.random_rows(N, 4, seed=100 + N), oc.params(N, **base)))
    with open(fin, "wb") as f:
        for _, rows, p in cases:
            R, N = rows.shape
            f.write(np.array([N, R, p["rank"], p["gap"], p["min_width"], p["max_emissions"], int(p["shift"])], np.int32).tobytes())
            f.write(np.array([p["factor"], p["min_level"]], np.float32).tobytes())
            f.write(np.ascontiguousarray(rows, np.float32).tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "occ law ok: %d cases" % len(cases) in r.stdout, r.stdout + r.stderr
    raw, at = np.fromfile(fout, np.uint8), 0
    for name, rows, p in cases:
        R, N = rows.shape
        E = p["max_emissions"]
        info = raw[at:at + 16 * R].view(synth.OCC_INFO)
        rec = raw[at + 16 * R:at + 16 * R + 32 * E * R].view(synth.OCC_REC).reshape(R, E)
        mask = raw[at + 16 * R + 32 * E * R:at + 16 * R + 32 * E * R + R * N].reshape(R, N)
        at += 16 * R + 32 * E * R + R * N
        same_bytes((info, rec, mask), synth.occ_reference(rows, **p), name)
    assert at == raw.size
