"""The Reed-Solomon outer code's host plan (sfe_dsp_reed_plan: csrc/reed_law.h compiled for the host -- Berlekamp-Massey, a root
search, Forney) against synth.reed_reference, the numpy restatement of the law (Peterson-Gorenstein-Zierler, every
correction kept only if it yields a codeword), byte for byte: the reference itself against a search over every word at
distance 1, then every shape and error pattern of tests/reed_cases.py, encode and decode.  Beyond-t inputs are asserted
equal to the reference, never assumed to fail.  Then the refusals, the build's bookkeeping, and the serial law through a
stand-alone program built with -fsanitize=address,undefined (tests/host/test_reed_law.cpp).  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import reed_cases as rc
from simplefe_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = sorted(rc.SHAPES)


@pytest.fixture(scope="module")
def api():
    from simplefe_amd import api as a, build
    build.build_lib()
    return a


@pytest.fixture(scope="module")
def L():
    from simplefe_amd import lib
    return lib


def same(got, want, what):
    for name, g, w in zip(("bytes", "record", "status"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        d = np.argwhere(g != w)
        assert d.size == 0, "%s: %s differs at %d places, the first at %s: %r != %r" % (what, name, len(d), d[0], g[tuple(d[0])], w[tuple(d[0])])


@pytest.mark.parametrize("shape", [(0x11d, 0, 1, 7, 2, 1), (0x187, 112, 11, 9, 3, 1)], ids=["7-2", "9-3"])
def test_the_reference_equals_a_search_over_distance_one(shape):
    """48 seeded words with 0 .. t + 2 = 3 wrong bytes: solving the syndromes and trying every word at distance 1 agree on
    the word returned and on the verdict."""
    prim, fcr, step, n, n_par, I = shape
    rng = np.random.default_rng(n)
    frames = synth.reed_reference(*shape, rc.payloads(shape, 48, 5), encode=True)
    for f in range(48):
        rc.hit(frames[f], 1, 0, rng.choice(n, size=f % 4, replace=False), rng)
    solved, searched = synth.reed_reference(*shape, frames), synth.reed_reference(*shape, frames, brute=True)
    same(solved, searched, str(shape))
    assert (solved[2] == 0).sum() >= 24 and (solved[2] == 1).any()     # 0 and 1 wrong bytes decode; some of the rest do not


@pytest.mark.parametrize("key", KEYS)
def test_the_plan_equals_the_reference(api, key):
    """Every pattern, with the whitening sequence and without: encode, then decode, in bytes, record and status."""
    shape = rc.SHAPES[key]
    rc.check_the_reference(key)
    for with_wh in (True, False):
        names, pay, frames, wh = rc.patterns(key, with_wh)
        enc = api.reed_plan(*shape, whiten=wh, data=pay, encode=True)
        want = synth.reed_reference(*shape, pay, whiten=wh, encode=True)
        assert enc.dtype == want.dtype and np.array_equal(enc, want), (key, with_wh)
        same(api.reed_plan(*shape, whiten=wh, data=frames), rc.reference(key, with_wh), "%s whitening %d" % (key, with_wh))


@pytest.mark.parametrize("key", KEYS)
def test_codewords_vanish_at_the_roots_and_carry_the_payload(api, key):
    """In the reference's arithmetic: every codeword of every encoded frame is zero at the n_par roots; frame[:P] is the
    payload; whitening commutes with encoding."""
    shape = rc.SHAPES[key]
    prim, fcr, step, n, n_par, I = shape
    P, Fb, t = rc.sizes(shape)
    pay, wh = rc.payloads(shape, 5, 31), rc.whitening(shape)
    assert api.reed_plan(*shape) == (P, Fb)
    plain = api.reed_plan(*shape, data=pay, encode=True)
    assert plain.shape == (5, Fb) and np.array_equal(plain[:, :P], pay)
    words = plain.reshape(5, n, I).transpose(0, 2, 1).reshape(5 * I, n)
    assert not synth.reed_syndromes(words, synth.reed_tables(prim, fcr, step, n, n_par)[0], prim).any()
    assert np.array_equal(api.reed_plan(*shape, whiten=wh, data=pay, encode=True), plain ^ wh[None, :])


def test_frames_marked_upstream_are_not_read(api):
    shape = rc.SHAPES["C"]
    P, Fb, t = rc.sizes(shape)
    frames, wh = rc.many("C", 6)
    si = [0, 3, 0, 0, -1, 0]
    got = api.reed_plan(*shape, whiten=wh, data=frames, status_in=si)
    same(got, synth.reed_reference(*shape, frames, whiten=wh, status_in=si), "status_in")
    clean = api.reed_plan(*shape, whiten=wh, data=frames)
    for b in range(6):
        if si[b]:
            assert not got[0][b].any() and got[1][b].tolist() == [0, 7] and got[2][b] == 2
        else:
            assert all(np.array_equal(g[b], c[b]) for g, c in zip(got, clean))


def test_each_output_of_the_plan_may_be_null(api, L):
    shape = rc.SHAPES["E"]
    P, Fb, t = rc.sizes(shape)
    frames, wh = rc.many("E", 12)
    by, rec, st = api.reed_plan(*shape, whiten=wh, data=frames)
    lib = L.load()
    head = (*shape, wh.ctypes.data, 0, frames.ctypes.data, Fb, None, 12)
    b2, r2, s2 = np.zeros_like(by), np.zeros_like(rec), np.zeros_like(st)
    assert lib.sfe_dsp_reed_plan(*head, b2.ctypes.data, P, None, None, None, None) == L.SFE_OK and np.array_equal(b2, by)
    assert lib.sfe_dsp_reed_plan(*head, None, 0, r2.ctypes.data, None, None, None) == L.SFE_OK and np.array_equal(r2, rec)
    assert lib.sfe_dsp_reed_plan(*head, None, 0, None, s2.ctypes.data, None, None) == L.SFE_OK and np.array_equal(s2, st)
    assert lib.sfe_dsp_reed_plan(*head, None, 0, None, None, None, None) == L.SFE_OK
    p, f = C.c_int(-1), C.c_int(-1)
    assert lib.sfe_dsp_reed_plan(*shape, None, 0, None, 0, None, 0, None, 0, None, None, C.byref(p), None) == L.SFE_OK and p.value == P
    assert lib.sfe_dsp_reed_plan(*shape, None, 1, None, 0, None, 0, None, 0, None, None, None, C.byref(f)) == L.SFE_OK and f.value == Fb


def test_refusals_and_their_prefix(api, L):
    lib = L.load()
    good = dict(prim=0x11d, fcr=1, step=1, n=40, n_par=8, depth=3)
    order = ("prim", "fcr", "step", "n", "n_par", "depth")
    tail = (None, 0, None, 0, None, 0, None, 0, None, None, None, None)
    assert lib.sfe_dsp_reed_plan(*[good[k] for k in order], *tail) == L.SFE_OK
    bad = [("prim", 0x11b), ("prim", 0xff), ("prim", 0x200), ("prim", 0x11c), ("fcr", -1), ("fcr", 255), ("step", 0), ("step", 3),
           ("step", 85), ("step", 255), ("n", 2), ("n", 256), ("n_par", 1), ("n_par", 40), ("n_par", 41), ("n_par", 65), ("depth", 0),
           ("depth", 17)]
    h = C.c_void_p(1)
    for k, v in bad:
        a = [dict(dict(good, n=255) if (k, v) == ("n_par", 65) else good, **{k: v})[name] for name in order]
        assert lib.sfe_dsp_reed_plan(*a, *tail) == L.SFE_EINVAL, (k, v)
        assert lib.sfe_dsp_last_error().startswith(b"reed: "), lib.sfe_dsp_last_error()
        # create refuses them before it looks for a device: SFE_EINVAL on a machine with no GPU too
        assert lib.sfe_dsp_reed_create(*a, None, 0, C.byref(h)) == L.SFE_EINVAL and h.value is None, (k, v)
        assert lib.sfe_dsp_last_error().startswith(b"reed: ")
        h.value = 1
    a = [good[k] for k in order]
    assert lib.sfe_dsp_reed_plan(*a, None, 2, *tail[2:]) == L.SFE_EINVAL and lib.sfe_dsp_last_error().startswith(b"reed: ")     # encode = 2
    P, Fb = 3 * 32, 3 * 40
    buf, res = np.zeros(4 * Fb, np.uint8), np.zeros(4 * Fb, np.uint8)
    for enc, istride, ostride in ((0, Fb - 1, P), (0, Fb, P - 1), (1, P - 1, Fb), (1, P, Fb - 1)):
        assert lib.sfe_dsp_reed_plan(*a, None, enc, buf.ctypes.data, istride, None, 2, res.ctypes.data, ostride, None, None, None, None) == L.SFE_ERANGE
        assert lib.sfe_dsp_last_error().startswith(b"reed: ")
    with pytest.raises(api.SfeError):
        api.reed_plan(0x11b, 1, 1, 40, 8, 3)
    with pytest.raises(ValueError):
        api.reed_plan(0x11d, 1, 1, 40, 8, 3, whiten=np.zeros(7, np.uint8))
    if not os.path.exists("/dev/kfd"):
        with pytest.raises(api.SfeError) as e:
            api.Reed(0x11d, 1, 1, 40, 8, 3)
        assert e.value.code == L.SFE_ENODEV
    k = C.c_size_t(5)
    assert lib.sfe_dsp_reed_process_stream(None, None, 120, None, 1, None, 96, None, None, C.byref(k), None) == L.SFE_EINVAL and k.value == 0
    assert lib.sfe_dsp_last_error().startswith(b"reed_process_stream: ")
    k.value = 5
    assert lib.sfe_dsp_reed_encode_stream(None, None, 96, 1, None, 120, C.byref(k), None) == L.SFE_EINVAL and k.value == 0
    assert lib.sfe_dsp_last_error().startswith(b"reed_encode_stream: ")
    assert lib.sfe_dsp_reed_destroy(None) == L.SFE_OK


def test_the_kernels_are_registered_and_touch_no_scratch(api):
    import json
    import re
    from simplefe_amd import build
    res = json.load(open(os.path.join(build.HERE, "build", "reed.hip.resources.json")))
    assert len(res) == 2 and sum("reed_decode_kernel" in k for k in res) == 1 and sum("reed_encode_kernel" in k for k in res) == 1
    for k, r in res.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (k, r)
        assert r["LDS Size"] <= 8 * 1024 and r["Occupancy"] >= 4, (k, r)
    assert "reed.hip" in build.EXACT_SOURCES and "api_reed.hip" in build.HOST_SOURCES and build.SCRATCH_FREE["reed.hip"]
    assert build.KERNEL_FILES["reed"] == ("reed.hip", "reed.h", "reed_law.h", "common.h")
    cm = open(os.path.join(ROOT, "CMakeLists.txt")).read()
    assert re.search(r"set\(SFE_EXACT_SOURCES [^)]*\breed\.hip\b", cm)


def test_the_law_under_the_sanitizers(tmp_path):
    """tests/host/test_reed_law.cpp, built with the host compiler and -fsanitize=address,undefined, runs the serial law over
    every shape's patterns -- encode and decode, with the whitening sequence, a status table on one case -- from heap blocks
    of exactly the contract's sizes; what it writes is the reference's, byte for byte."""
    exe, fin, fout = str(tmp_path / "reed_law"), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    r = subprocess.run(["g++", "-O1", "-Wall", "-std=c++14", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests/host/test_reed_law.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    cases = []                                          # (shape, encode, whitening, status_in, rows, what the reference gives)
    for key in KEYS:
        names, pay, frames, wh = rc.patterns(key)
        cases.append((rc.SHAPES[key], True, wh, None, pay, synth.reed_reference(*rc.SHAPES[key], pay, whiten=wh, encode=True)))
        cases.append((rc.SHAPES[key], False, wh, None, frames, rc.reference(key)))
    names, pay, frames, _ = rc.patterns("C", False)
    si = (np.arange(frames.shape[0]) % 3 == 1).astype(np.int32)
    cases.append((rc.SHAPES["C"], False, None, si, frames, synth.reed_reference(*rc.SHAPES["C"], frames, status_in=si)))
    with open(fin, "wb") as f:
        for shape, enc, wh, si, rows, _ in cases:
            f.write(np.array([*shape, rows.shape[0], int(enc) | 2 * (wh is not None) | 4 * (si is not None)], np.int32).tobytes())
            if wh is not None:
                f.write(wh.tobytes())
            if si is not None:
                f.write(si.tobytes())
            f.write(np.ascontiguousarray(rows, np.uint8).tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "reed law ok: %d cases" % len(cases) in r.stdout, r.stdout + r.stderr
    raw, at = np.fromfile(fout, np.uint8), 0
    for shape, enc, wh, si, rows, want in cases:
        P, Fb, t = rc.sizes(shape)
        nf = rows.shape[0]
        if enc:
            got = raw[at:at + nf * Fb].reshape(nf, Fb)
            at += nf * Fb
            assert np.array_equal(got, want), shape
        else:
            by = raw[at:at + nf * P].reshape(nf, P)
            rec = raw[at + nf * P:at + nf * P + 8 * nf].view(np.uint32).reshape(nf, 2)
            st = raw[at + nf * P + 8 * nf:at + nf * P + 12 * nf].view(np.int32)
            at += nf * (P + 12)
            same((by, rec, st), want, str(shape))
    assert at == raw.size
