"""The quasi-cyclic LDPC code's host plan (sfe_dsp_ldpc_plan: csrc/ldpc_law.h compiled for the host, layer by layer over the
cell table) against synth.ldpc_reference, the numpy restatement of the law on the expanded matrix, which knows nothing of
circulants or layers: the reference itself against a literal transcription of the law on the Hamming code, then every code,
input group, special word, parameter set and input mode of tests/ldpc_cases.py, in bytes, record and status.  Then
encoding, the null outputs, the refusals, the bound on |APP|, the build's bookkeeping, and the serial law through a
stand-alone program built with -fsanitize=address,undefined (tests/host/test_ldpc_law.cpp).  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ldpc_cases as lc
from simplefe_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = sorted(lc.CASES)


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


def direct(rows, Lq, a, beta, max_iter):
    """The law as include/sfe_dsp.h words it, on plain Python integers: (APP, iterations, unsatisfied checks)."""
    app = [int(v) for v in Lq]
    R = {(r, int(v)): 0 for r, cols in enumerate(rows) for v in cols}

    def unsatisfied():
        return sum(sum(app[v] < 0 for v in cols) & 1 for cols in rows)

    it, u = 0, unsatisfied()
    while u and it < max_iter:
        for r, cols in enumerate(rows):
            cols = [int(v) for v in cols]
            Q = [app[v] - R[r, v] for v in cols]
            mags = [abs(q) for q in Q]
            m1 = min(mags)
            js = mags.index(m1)
            m2 = min(m for j, m in enumerate(mags) if j != js)
            S = sum(q < 0 for q in Q) & 1
            for j, v in enumerate(cols):
                Mp = min(max((((m2 if j == js else m1) * a) >> 4) - beta, 0), 127)
                Rn = -Mp if (S ^ (Q[j] < 0)) else Mp
                app[v], R[r, v] = Q[j] + Rn, Rn
        it, u = it + 1, unsatisfied()
    return app, it, u


@pytest.mark.parametrize("pset", sorted(lc.PARAMS))
def test_the_reference_equals_a_direct_statement_on_the_hamming_code(pset):
    """All 16 codewords x {no flip, each single flip} x two magnitude patterns."""
    s, Z = lc.CASES["H"]
    a, beta, max_iter = lc.PARAMS[pset]
    rows = synth.ldpc_expand(s, Z)
    pay = (np.arange(16, dtype=np.uint8) << 4).reshape(16, 1)
    bits = np.unpackbits(synth.ldpc_encode_reference(s, Z, pay), axis=1)[:, :7]
    H = synth.ldpc_dense(rows, 7)
    assert not ((H @ bits.T) & 1).any() and len({tuple(b) for b in bits.tolist()}) == 16 and np.array_equal(bits[:, :4], np.unpackbits(pay, axis=1)[:, :4])
    x, sent = [], []
    for mags in (np.ones(7), np.array([0.3, 1.1, 0.7, 2.0, 0.45, 1.6, 0.9])):
        for w in range(16):
            for flip in range(-1, 7):
                r = (1.0 - 2.0 * bits[w]) * mags
                if flip >= 0:
                    r[flip] = -r[flip]
                x.append(r), sent.append(w)
    x = np.array(x, np.float32)
    by, rec, st = synth.ldpc_reference(s, Z, x, lc.SCALE, a, beta, max_iter)
    one = synth.ldpc_reference(s, Z, x, lc.SCALE, a, beta, max_iter, one_at_a_time=True)
    same((by, rec, st), one, "runs of rows against single rows")
    for i in range(x.shape[0]):
        Lq = synth.ldpc_quantise(x[i], lc.SCALE)
        app, it, u = direct(rows, Lq, a, beta, max_iter)
        hard = np.array([v < 0 for v in app], np.uint8)
        assert by[i, 0] == np.packbits(hard[:4])[0] and rec[i].tolist() == [it, u, int(((Lq != 0) & (hard != (Lq < 0))).sum())], i
        assert st[i] == (0 if u == 0 else 3), i
        if i % 8 == 0:          # no flip: a codeword as it was sent
            assert rec[i].tolist() == [0, 0, 0] and by[i, 0] == pay[sent[i], 0]


@pytest.mark.parametrize("key", ["A", "B", "G"])
def test_runs_of_commuting_rows_are_the_rows_one_at_a_time(key):
    """The reference updates consecutive rows that share no variable in one numpy step; walking every row alone gives the
    same bytes, records and statuses."""
    s, Z = lc.CASES[key]
    x = lc.inputs(key)[1]
    for pset, (a, beta, max_iter) in lc.PARAMS.items():
        same(lc.reference(key, pset)[:3], synth.ldpc_reference(s, Z, x, lc.SCALE, a, beta, max_iter, one_at_a_time=True), key + pset)


@pytest.mark.parametrize("pset", sorted(lc.PARAMS))
@pytest.mark.parametrize("key", KEYS)
def test_the_plan_equals_the_reference(api, L, key, pset):
    """Every group and special word, in all three input modes and with skip > 0: bytes, record and status."""
    s, Z = lc.CASES[key]
    a, beta, max_iter = lc.PARAMS[pset]
    lc.check_the_reference(key, pset)
    x, want = lc.inputs(key)[1], lc.reference(key, pset)[:3]
    same(api.ldpc_plan(s, Z, lc.SCALE, a, beta, max_iter, x=x), want, key + pset)
    for mode, skip in ((L.VIT_IN_BPSK, 0), (L.VIT_IN_BPSK, 5), (L.VIT_IN_QPSK, 0), (L.VIT_IN_QPSK, 3)):
        got = api.ldpc_plan(s, Z, lc.SCALE, a, beta, max_iter, in_mode=mode, skip=skip, x=lc.as_mode(x, mode, skip))
        same(got, want, "%s %s mode %d skip %d" % (key, pset, mode, skip))


def test_words_marked_upstream_are_not_read(api):
    s, Z = lc.CASES["C"]
    x = lc.inputs("C")[1].copy()
    si = (np.arange(x.shape[0]) % 4 == 1).astype(np.int32) * -3
    clean = api.ldpc_plan(s, Z, lc.SCALE, 12, 0, 32, x=x)
    x[si != 0] = np.nan
    got = api.ldpc_plan(s, Z, lc.SCALE, 12, 0, 32, x=x, status_in=si)
    same(got, synth.ldpc_reference(s, Z, x, lc.SCALE, 12, 0, 32, status_in=si), "status_in")
    for b in range(x.shape[0]):
        if si[b]:
            assert not got[0][b].any() and not got[1][b].any() and got[2][b] == 2
        else:
            assert all(np.array_equal(g[b], c[b]) for g, c in zip(got, clean))


@pytest.mark.parametrize("key", lc.ENCODABLE)
def test_codewords_carry_the_payload_and_have_a_zero_syndrome(api, key):
    """The whole law of encoding: c[0 .. k) is the payload, H c = 0 under the expanded H, pad bits are 0 -- and, the
    codeword being unique, the plan's bytes are the reference's."""
    s, Z = lc.CASES[key]
    n, k, kb, nb = lc.sizes(key)
    assert api.ldpc_plan(s, Z) == (n, k, True)
    pay = lc.payloads(key, 5, 31)
    pay[0] = 0
    pay[1] = 255
    code = api.ldpc_plan(s, Z, data=pay)
    assert code.shape == (5, nb) and code.dtype == np.uint8
    bits = np.unpackbits(code, axis=1)
    assert np.array_equal(bits[:, :k], np.unpackbits(pay, axis=1)[:, :k]) and not bits[:, n:].any()
    for cols in synth.ldpc_expand(s, Z):
        assert not (bits[:, cols].sum(axis=1) & 1).any()
    assert not code[0].any()
    assert np.array_equal(code, synth.ldpc_encode_reference(s, Z, pay))


def test_a_singular_parity_part_is_not_encodable(api, L):
    s, Z = lc.CASES["G"]
    assert not synth.ldpc_encodable(s, Z) and synth.ldpc_encodable(*lc.CASES["A"])
    assert api.ldpc_plan(s, Z) == (42, 21, False)
    with pytest.raises(api.SfeError) as e:
        api.ldpc_plan(s, Z, data=lc.payloads("G", 2, 1))
    assert e.value.code == L.SFE_ESTATE and "ldpc: " in str(e.value)


def test_each_output_of_the_plan_may_be_null(api, L):
    s, Z = lc.CASES["B"]
    n, k, kb, nb = lc.sizes("B")
    x = lc.inputs("B")[1]
    W = x.shape[0]
    by, rec, st = api.ldpc_plan(s, Z, lc.SCALE, 12, 0, 32, x=x)
    lib = L.load()
    sh = np.ascontiguousarray(s, np.int16)
    head = (12, 24, Z, sh.ctypes.data, lc.SCALE, 12, 0, 32, 0, 0, 0, x.ctypes.data, n, None, W)
    b2, r2, s2 = np.zeros_like(by), np.zeros_like(rec), np.zeros_like(st)
    assert lib.sfe_dsp_ldpc_plan(*head, b2.ctypes.data, kb, None, None, None, None, None) == L.SFE_OK and np.array_equal(b2, by)
    assert lib.sfe_dsp_ldpc_plan(*head, None, 0, r2.ctypes.data, None, None, None, None) == L.SFE_OK and np.array_equal(r2, rec)
    assert lib.sfe_dsp_ldpc_plan(*head, None, 0, None, s2.ctypes.data, None, None, None) == L.SFE_OK and np.array_equal(s2, st)
    assert lib.sfe_dsp_ldpc_plan(*head, None, 0, None, None, None, None, None) == L.SFE_OK
    pay = lc.payloads("B", 2, 9)
    assert lib.sfe_dsp_ldpc_plan(*head[:10], 1, pay.ctypes.data, kb, None, 2, None, 0, None, None, None, None, None) == L.SFE_OK
    v = C.c_int(-1)
    tail = (0, None, 0, None, 0, None, 0, None, None)
    assert lib.sfe_dsp_ldpc_plan(*head[:10], *tail, C.byref(v), None, None) == L.SFE_OK and v.value == n
    assert lib.sfe_dsp_ldpc_plan(*head[:10], *tail, None, C.byref(v), None) == L.SFE_OK and v.value == k
    assert lib.sfe_dsp_ldpc_plan(*head[:10], *tail, None, None, C.byref(v)) == L.SFE_OK and v.value == 1
    assert api.ldpc_footprint(s, Z) == (api.ldpc_footprint(s, Z)[0], 4) and api.ldpc_footprint(*lc.CASES["F"])[1] == 1


def test_refusals_and_their_prefix(api, L):
    """Every limit one step beyond."""
    lib = L.load()
    good = lc.qc(3, 6, 7, 101, 2)

    def plan(s, Z, scale=8.0, a=12, beta=0, max_iter=32, in_mode=0, skip=0, encode=0, mb=None, nb=None, null=False):
        s = np.ascontiguousarray(s, np.int16)
        args = (s.shape[0] if mb is None else mb, s.shape[1] if nb is None else nb, Z, None if null else s.ctypes.data, scale, a, beta, max_iter,
                in_mode, skip)
        rc = lib.sfe_dsp_ldpc_plan(*args, encode, None, 0, None, 0, None, 0, None, None, None, None, None)
        if rc != L.SFE_OK:
            assert lib.sfe_dsp_last_error().startswith(b"ldpc: "), lib.sfe_dsp_last_error()
            # create refuses the same before it looks for a device: SFE_EINVAL on a machine with no GPU too
            h = C.c_void_p(1)
            if encode in (0, 1):        # (create has no such argument)
                assert lib.sfe_dsp_ldpc_create(*args, 0, C.byref(h)) == rc and h.value is None and lib.sfe_dsp_last_error().startswith(b"ldpc: ")
        return rc

    def full(mb, nb, Z=1):
        return np.zeros((mb, nb), np.int16)

    assert plan(good, 7) == L.SFE_OK
    assert plan(full(2, 3), 512) == L.SFE_OK and plan(full(2, 3), 513) == L.SFE_EINVAL and plan(full(2, 3), 0) == L.SFE_EINVAL       # Z
    wide = np.full((64, 128), -1, np.int16)
    wide[:, :64], wide[:, 64:] = np.where(np.eye(64, dtype=bool), 0, -1), np.where(np.eye(64, dtype=bool), 0, -1)
    assert plan(wide, 64) == L.SFE_OK                                                   # mb = 64, n = 8192: the limits themselves
    assert plan(wide, 65) == L.SFE_EINVAL                                               # n = 8320
    tall = np.full((65, 130), -1, np.int16)
    tall[:, :65], tall[:, 65:] = np.where(np.eye(65, dtype=bool), 0, -1), np.where(np.eye(65, dtype=bool), 0, -1)
    assert plan(tall, 1) == L.SFE_EINVAL                                                # mb = 65
    assert plan(good, 7, mb=0) == L.SFE_EINVAL and plan(full(3, 3), 1) == L.SFE_EINVAL and plan(full(3, 2), 1) == L.SFE_EINVAL     # mb < 1, nb <= mb
    long_row = np.full((2, 257), -1, np.int16)
    long_row[0, :128], long_row[1, 128:], long_row[0, 256], long_row[1, 0] = 0, 0, 0, 0
    assert plan(long_row[:, :256], 1) == L.SFE_EINVAL                                   # a row of 128 cells at nb = 256
    assert plan(long_row, 1) == L.SFE_EINVAL                                            # nb = 257
    assert plan(full(2, 32), 1) == L.SFE_OK and plan(full(2, 33), 1) == L.SFE_EINVAL    # 32 cells in a row, then 33
    thin = full(2, 3)
    thin[1, :2] = -1
    assert plan(thin, 1) == L.SFE_EINVAL                                                # a row of one cell
    gap = full(2, 4)
    gap[:, 2] = -1
    assert plan(gap, 1) == L.SFE_EINVAL                                                 # a block column without a cell
    bad = good.copy()
    bad[0, np.flatnonzero(good[0] >= 0)[0]] = 7
    assert plan(bad, 7) == L.SFE_EINVAL                                                 # shift = Z
    bad[0, np.flatnonzero(good[0] >= 0)[0]] = -2
    assert plan(bad, 7) == L.SFE_EINVAL                                                 # shift = -2
    assert plan(good, 7, null=True) == L.SFE_EINVAL
    assert plan(full(8, 16), 512) == L.SFE_OK                                           # 128 cells x 512 = 65 536 edges: the limit itself
    assert plan(full(9, 16), 512) == L.SFE_EINVAL                                       # 144 cells x 512
    for kw in (dict(scale=0.0), dict(scale=-1.0), dict(scale=float("inf")), dict(scale=float("nan")), dict(a=0), dict(a=17), dict(beta=-1),
               dict(beta=128), dict(max_iter=0), dict(max_iter=65), dict(in_mode=3), dict(in_mode=-1), dict(skip=-1), dict(skip=(1 << 24) + 1),
               dict(skip=1), dict(encode=2)):
        assert plan(good, 7, **kw) == L.SFE_EINVAL, kw
    assert plan(good, 7, a=1, beta=127, max_iter=64, in_mode=1, skip=1 << 24) == L.SFE_OK and plan(good, 7, a=16, max_iter=1) == L.SFE_OK
    sh = np.ascontiguousarray(good, np.int16)
    head = (3, 6, 7, sh.ctypes.data, 8.0, 12, 0, 32)
    x, res = np.zeros(4 * 64, np.float32), np.zeros(64, np.uint8)
    for mode, skip, encode, istride, ostride in ((0, 0, 0, 41, 3), (0, 0, 0, 42, 2), (1, 2, 0, 43, 3), (2, 2, 0, 22, 3), (0, 0, 1, 2, 6), (0, 0, 1, 3, 5)):
        rc = lib.sfe_dsp_ldpc_plan(*head, mode, skip, encode, x.ctypes.data, istride, None, 2, res.ctypes.data, ostride, None, None, None, None, None)
        assert rc == L.SFE_ERANGE and lib.sfe_dsp_last_error().startswith(b"ldpc: "), (mode, skip, encode)
    assert lib.sfe_dsp_ldpc_plan(*head, 0, 0, 0, x.ctypes.data, 42, None, 1 << 31, res.ctypes.data, 3, None, None, None, None, None) == L.SFE_EINVAL
    with pytest.raises(api.SfeError):
        api.ldpc_plan(good, 6)                                       # the matrix holds a shift of 6
    with pytest.raises(ValueError):
        api.ldpc_plan(np.zeros(6, np.int16), 1)
    if not os.path.exists("/dev/kfd"):
        with pytest.raises(api.SfeError) as e:
            api.Ldpc(good, 7)
        assert e.value.code == L.SFE_ENODEV
    k = C.c_size_t(5)
    assert lib.sfe_dsp_ldpc_process_stream(None, None, 42, None, 1, None, 3, None, None, C.byref(k), None) == L.SFE_EINVAL and k.value == 0
    assert lib.sfe_dsp_last_error().startswith(b"ldpc_process_stream: ")
    k.value = 5
    assert lib.sfe_dsp_ldpc_encode_stream(None, None, 3, 1, None, 6, C.byref(k), None) == L.SFE_EINVAL and k.value == 0
    assert lib.sfe_dsp_last_error().startswith(b"ldpc_encode_stream: ")
    assert lib.sfe_dsp_ldpc_destroy(None) == L.SFE_OK


@pytest.mark.parametrize("key", KEYS)
def test_the_sums_stay_inside_the_bound(key):
    """Over all the case's inputs and both parameter sets: |APP| <= 127 (1 + the largest column degree)."""
    s, Z = lc.CASES[key]
    bound = 127 * (1 + int((s >= 0).sum(axis=0).max()))
    for pset in lc.PARAMS:
        peak = lc.reference(key, pset)[3]
        assert 0 < peak <= bound <= 127 * 65, (key, pset, peak, bound)


def test_the_kernels_are_registered_and_touch_no_scratch(api):
    import json
    import re
    from simplefe_amd import build
    res = json.load(open(os.path.join(build.HERE, "build", "ldpc.hip.resources.json")))
    assert len(res) == 2 and sum("ldpc_decode_kernel" in k for k in res) == 1 and sum("ldpc_encode_kernel" in k for k in res) == 1
    for k, r in res.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (k, r)
        assert r["LDS Size"] == 0 and r["Occupancy"] >= 4, (k, r)           # all of the LDS is the launch's
    assert "ldpc.hip" in build.EXACT_SOURCES and "api_ldpc.hip" in build.HOST_SOURCES and build.SCRATCH_FREE["ldpc.hip"]
    assert build.KERNEL_FILES["ldpc"] == ("ldpc.hip", "ldpc.h", "ldpc_law.h", "common.h")
    cm = open(os.path.join(ROOT, "CMakeLists.txt")).read()
    assert re.search(r"set\(SFE_EXACT_SOURCES [^)]*\bldpc\.hip\b", cm)


def test_the_law_under_the_sanitizers(tmp_path):
    """tests/host/test_ldpc_law.cpp, built with the host compiler and -fsanitize=address,undefined, runs the serial law over
    cases A, B and D -- decode with both parameter sets, a status table on one case, and encode -- from heap blocks of exactly
    the contract's sizes; what it writes is the reference's, byte for byte."""
    exe, fin, fout = str(tmp_path / "ldpc_law"), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    r = subprocess.run(["g++", "-O1", "-Wall", "-std=c++14", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tests/host/test_ldpc_law.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    cases = []                                          # (key, (a, beta, max_iter), encode, status_in, rows, what the reference gives)
    for key in "ABD":
        s, Z = lc.CASES[key]
        for pset, par in lc.PARAMS.items():
            cases.append((key, par, False, None, lc.inputs(key)[1], lc.reference(key, pset)[:3]))
        pay = lc.payloads(key, 4, 21)
        cases.append((key, lc.PARAMS["a12"], True, None, pay, synth.ldpc_encode_reference(s, Z, pay)))
    x = lc.inputs("B")[1]
    si = (np.arange(x.shape[0]) % 3 == 1).astype(np.int32)
    cases.append(("B", lc.PARAMS["a12"], False, si, x, synth.ldpc_reference(*lc.CASES["B"], x, lc.SCALE, 12, 0, 32, status_in=si)))
    with open(fin, "wb") as f:
        for key, par, enc, si, rows, _ in cases:
            s, Z = lc.CASES[key]
            f.write(np.array([s.shape[0], s.shape[1], Z, *par, rows.shape[0], int(enc) | 4 * (si is not None)], np.int32).tobytes())
            f.write(np.float32(lc.SCALE).tobytes())
            f.write(np.ascontiguousarray(s, np.int16).tobytes())
            if si is not None:
                f.write(si.tobytes())
            f.write(np.ascontiguousarray(rows).tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ldpc law ok: %d cases" % len(cases) in r.stdout, r.stdout + r.stderr
    raw, at = np.fromfile(fout, np.uint8), 0
    for key, par, enc, si, rows, want in cases:
        n, k, kb, nb = lc.sizes(key)
        nw = rows.shape[0]
        if enc:
            got = raw[at:at + nw * nb].reshape(nw, nb)
            at += nw * nb
            assert np.array_equal(got, want), key
        else:
            by = raw[at:at + nw * kb].reshape(nw, kb)
            rec = raw[at + nw * kb:at + nw * kb + 12 * nw].view(np.uint32).reshape(nw, 3)
            st = raw[at + nw * kb + 12 * nw:at + nw * kb + 16 * nw].view(np.int32)
            at += nw * (kb + 16)
            same((by, rec, st), want, key)
    assert at == raw.size
