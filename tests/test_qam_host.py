"""The QAM mapper and soft demapper (sfe_dsp_qam_*) without a GPU: the C ABI's declarations and exports, the build lists,
the refusals of the plan and of create, the constellation, the host plan against a restatement of the law in numpy float32
(bit equality) and against the float64 brute-force reference synth.qam_reference, the round trip, the exact case, the law
header under the sanitizers, the kernels' resources, and the chain through the plans.

The bar against float64 is derived from the law's roundings, not measured: |r - r_ref| <= 8 * 2^-24 * w * (D0 + D1) --
three half-ulp roundings in each e (the difference, its square counted twice), one in D1 - D0, one in the product with w,
and the roundings of w itself under CSI.  The worst ratio to the bar is printed."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import ldpc_cases as lc
import ofdmmod_cases as mc
import qam_cases as qc
from simplefe_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "sfe_dsp.h")
QAM_FUNCS = ("sfe_dsp_qam_plan", "sfe_dsp_qam_create", "sfe_dsp_qam_map_stream", "sfe_dsp_qam_demap_stream", "sfe_dsp_qam_destroy")
F32 = np.float32


@pytest.fixture(scope="module")
def L():
    from simplefe_amd import lib
    return lib.load()


@pytest.fixture(scope="module")
def api():
    from simplefe_amd import api as a
    return a


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ ABI and build lists
def test_header_declares_qam_abi_and_library_exports_it(L):
    from simplefe_amd import lib
    hdr = open(HDR).read()
    assert set(re.findall(r"\b(sfe_dsp_qam_[a-z0-9_]+)\s*\(", hdr)) == set(QAM_FUNCS)
    assert {n for n in lib.SIGNATURES if n.startswith("sfe_dsp_qam_")} == set(QAM_FUNCS)
    for name in QAM_FUNCS:
        assert hasattr(L, name), name
    for name, v in (("SFE_QAM_MAP", 0), ("SFE_QAM_DEMAP", 1)):
        assert re.search(r"#define %s %d\b" % (name, v), hdr), name
    assert (lib.QAM_MAP, lib.QAM_DEMAP) == (0, 1)


def test_qam_sources_are_in_the_build_lists():
    from simplefe_amd import build
    assert "qam.hip" in build.EXACT_SOURCES and "api_qam.hip" in build.HOST_SOURCES
    assert build.KERNEL_FILES["qam"] == ("qam.hip", "qam.h", "qam_law.h", "common.h")
    assert build.SCRATCH_FREE["qam.hip"] == "QAM-mapper"
    cm = open(os.path.join(ROOT, "CMakeLists.txt")).read()
    assert re.search(r"set\(SFE_EXACT_SOURCES [^)]*\bqam\.hip\b", cm)
    for f in build.KERNEL_FILES["qam"] + ("api_qam.hip",):
        assert os.path.exists(os.path.join(build.CSRC, f)), f
    for f in ("qam.hip", "api_qam.hip"):        # one law, compiled by both sides (qam.hip through qam.h)
        text = open(os.path.join(build.CSRC, f)).read()
        assert '#include "qam_law.h"' in text or '#include "qam.h"' in text, f
    assert '#include "qam_law.h"' in open(os.path.join(build.CSRC, "qam.h")).read()
    law = open(os.path.join(build.CSRC, "qam_law.h")).read()
    assert law.count("#pragma clang fp contract(off)") >= 5        # every function that computes


def test_qam_kernels_use_no_scratch_and_the_lds_they_state():
    from simplefe_amd import build
    build.build_lib()
    res = json.load(open(os.path.join(build.HERE, "build", "qam.hip.resources.json")))
    demap = {tuple(a.strip() for a in re.search(r"qam_demap_kernel<(.*?)>", k).group(1).split(",")) for k in res if "qam_demap_kernel<" in k}
    mapk = {tuple(a.strip() for a in re.search(r"qam_map_kernel<(.*?)>", k).group(1).split(",")) for k in res if "qam_map_kernel<" in k}
    tf = ("false", "true")
    assert demap == {(str(b), c, p) for b in (1, 2, 4, 6, 8) for c in tf for p in tf}
    assert mapk == {(str(b), p) for b in (1, 2, 4, 6, 8) for p in tf}
    for k, v in res.items():
        assert v.get("ScratchSize", 1) == 0 and v.get("VGPRs Spill", 0) == 0 and v.get("SGPRs Spill", 0) == 0, (k, v)
        if "qam_map_kernel<" in k:
            want = 64                           # the level table
        else:                                   # the weights of a tile's residues; the floats of four waves at bps 6 and 8 without perm
            bps, csi, perm = re.search(r"qam_demap_kernel<(\d+), (\w+), (\w+)>", k).groups()
            group = {"1": 4, "2": 4, "4": 4, "6": 12, "8": 8}[bps]
            want = (16384 if csi == "true" else 0) + (256 * group * 4 if perm == "false" and group > 4 else 0)
        assert v.get("LDS Size", -1) == want, (k, v)
    print("qam kernels: VGPRs %d..%d, SGPRs up to %d" % (min(v["VGPRs"] for v in res.values()), max(v["VGPRs"] for v in res.values()),
                                                        max(v["TotalSGPRs"] for v in res.values())))


# ------------------------------------------------------------------------------------------------ refusals
def _shape(order=16, amp=1.0, scale=1.0, n_sym=6, perm=None, period=0, clen=0, idx=None):
    perm = None if perm is None else np.ascontiguousarray(perm, np.uint32)
    idx = None if idx is None else np.ascontiguousarray(idx, np.uint32)
    return (order, amp, scale, n_sym, None if perm is None else perm.ctypes.data, period, clen, None if idx is None else idx.ctypes.data), (perm, idx)


B24 = np.arange(24, dtype=np.uint32)
REFUSALS = [("order 8", dict(order=8)), ("order 0", dict(order=0)), ("order 1024", dict(order=1024)),
            ("amp 0", dict(amp=0.0)), ("a negative amp", dict(amp=-1.0)), ("a NaN amp", dict(amp=float("nan"))), ("an infinite amp", dict(amp=float("inf"))),
            ("scale 0", dict(scale=0.0)), ("a negative scale", dict(scale=-2.0)), ("a NaN scale", dict(scale=float("nan"))),
            ("an infinite scale", dict(scale=float("inf"))),
            ("a perm with a repeat", dict(perm=np.where(B24 == 7, 8, B24))), ("a perm entry at B", dict(perm=np.where(B24 == 3, 24, B24))),
            ("a csi_index at csi_len", dict(period=3, clen=5, idx=[0, 5, 1])), ("csi_period 4097", dict(period=4097, clen=8, idx=np.zeros(4097))),
            ("a negative csi_period", dict(period=-1)), ("csi_len 0", dict(period=2, clen=0, idx=[0, 0])), ("csi_len 65537", dict(period=1, clen=65537, idx=[0])),
            ("a null csi_index", dict(period=2, clen=4)),
            ("n_sym 0", dict(n_sym=0)), ("n_sym above 2^24", dict(n_sym=(1 << 24) + 1))]


@pytest.mark.parametrize("why,kw", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_plan_and_create_refuse_before_the_device_is_touched(L, why, kw):
    from simplefe_amd import lib
    head, _alive = _shape(**kw)
    bps, nb = C.c_int(9), C.c_size_t(9)
    assert L.sfe_dsp_qam_plan(*head, lib.QAM_MAP, None, 0, None, 0, 0, None, 0, C.byref(bps), C.byref(nb)) == lib.SFE_EINVAL, why
    assert L.sfe_dsp_last_error().startswith(b"qam: "), (why, L.sfe_dsp_last_error())
    assert bps.value == 0 and nb.value == 0
    h = C.c_void_p()
    assert L.sfe_dsp_qam_create(*head, 0, C.byref(h)) == lib.SFE_EINVAL, why
    assert L.sfe_dsp_last_error().startswith(b"qam: ") and not h.value, (why, L.sfe_dsp_last_error())


def test_plan_reports_and_refuses_its_buffers(L, api):
    from simplefe_amd import lib
    assert [api.qam_plan(M, 5) for M in qc.ORDERS] == [(1, 1), (2, 2), (4, 3), (6, 4), (8, 5)]
    assert api.qam_plan(64, 1 << 24) == (6, 6 << 21)
    head, _alive = _shape(n_sym=6, period=2, clen=3, idx=[2, 0])
    z, h, out = np.zeros(6, np.complex64), np.ones(3, np.complex64), np.full(24, 7.0, F32)

    def plan(direction=lib.QAM_DEMAP, pi=z.ctypes.data, istride=6, pc=h.ctypes.data, cstride=3, n=1, po=out.ctypes.data, ostride=24, hd=head):
        return L.sfe_dsp_qam_plan(*hd, direction, pi, istride, pc, cstride, n, po, ostride, None, None)

    for why, rc in (("a short in_stride", plan(istride=5)), ("a short out_stride", plan(ostride=23)), ("a short csi_stride", plan(cstride=2))):
        assert rc == lib.SFE_ERANGE and L.sfe_dsp_last_error().startswith(b"qam: "), why
    for why, rc in (("direction 2", plan(direction=2)), ("a null output", plan(po=None)), ("no csi on a csi shape", plan(pc=None)),
                    ("csi on a shape without", plan(hd=_shape(n_sym=6)[0]))):
        assert rc == lib.SFE_EINVAL and L.sfe_dsp_last_error().startswith(b"qam: "), why
    assert np.array_equal(out, np.full(24, 7.0, F32))
    assert plan(n=0) == lib.SFE_OK and plan(pi=None) == lib.SFE_OK and np.array_equal(out, np.full(24, 7.0, F32))
    assert plan() == lib.SFE_OK and not np.array_equal(out, np.full(24, 7.0, F32))


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present: create succeeds there")
def test_create_without_gpu_is_enodev():
    from simplefe_amd import api, lib
    with pytest.raises(lib.SfeError) as e:
        api.Qam(16, 10, perm=qc.perm_of("random", 40))
    assert e.value.code == lib.SFE_ENODEV


def test_null_handles_are_refused(L):
    from simplefe_amd import lib
    k = C.c_size_t(5)
    assert L.sfe_dsp_qam_map_stream(None, None, 4, 1, None, 4, C.byref(k), None) == lib.SFE_EINVAL
    assert L.sfe_dsp_last_error().startswith(b"qam_map_stream: ") and k.value == 0
    k = C.c_size_t(5)
    assert L.sfe_dsp_qam_demap_stream(None, None, 4, None, 0, 1, None, 4, C.byref(k), None) == lib.SFE_EINVAL
    assert L.sfe_dsp_last_error().startswith(b"qam_demap_stream: ") and k.value == 0
    assert L.sfe_dsp_qam_destroy(None) == lib.SFE_OK


# ------------------------------------------------------------------------------------------------ the constellation
@pytest.mark.parametrize("order", qc.ORDERS)
def test_the_constellation(api, order):
    """All 2^bps words through the mapper: distinct points, neighbours along each axis one bit apart, mean energy amp^2 within
    4 * 2^-24 relative, the components the law's table words; the axis order of m = 2."""
    bps, m = qc.BPS[order], qc.axis_bits(order)
    amp = F32(0.7)
    M = 1 << bps
    words = ((np.arange(M)[:, None] >> (bps - 1 - np.arange(bps))) & 1).astype(np.uint8)         # word p's bits, c = 0 first
    pts = api.qam_plan(order, M, amp=amp, data=np.packbits(words.ravel()))[0]
    assert np.unique(pts).size == M
    energy = float(np.mean(pts.real.astype(np.float64) ** 2 + pts.imag.astype(np.float64) ** 2))
    rel = abs(energy / float(amp) ** 2 - 1.0)
    print("order %d: mean energy off amp^2 by %.3e relative (bar %.3e)" % (order, rel, 4 * 2.0 ** -24))
    assert rel <= 4 * 2.0 ** -24
    lev = synth.qam_levels(order, amp)
    K = 1 if order == 2 else 2 * (order - 1) // 3
    u, _ = synth.qam_axis_words(m)
    assert np.array_equal(_bits(lev), _bits((np.float64(amp) * u / np.sqrt(np.float64(K))).astype(F32)))
    wi, wq = (np.arange(M), np.zeros(M, int)) if bps == 1 else np.divmod(np.arange(M), 1 << m)
    assert np.array_equal(_bits(pts.real), _bits(lev[wi]))
    assert np.array_equal(_bits(pts.imag), _bits(np.zeros(M, F32) if bps == 1 else lev[wq]))
    # along an axis: sort the points of one row / column by their level; neighbours differ in exactly one of the bps bits
    for axis, other in ((pts.real, pts.imag), (pts.imag, pts.real))[:1 if bps == 1 else 2]:
        for v in np.unique(other):
            line = np.flatnonzero(other == v)
            line = line[np.argsort(axis[line])]
            assert line.size == 1 << m
            assert (np.abs(words[line[1:]].astype(int) - words[line[:-1]].astype(int)).sum(axis=1) == 1).all()
    if m == 2:
        assert [int(w) for w in np.argsort(lev)] == [0b11, 0b10, 0b00, 0b01] and np.array_equal(np.sign(lev), [1, 1, -1, -1])


def test_order_4_is_the_ofdm_modulators_gray_qpsk(api):
    """M = 4 equals ofdmmod_plan's BITS-mode bins bit for bit.  The two levels are +-float32(amp / sqrt 2), the modulator's a4, at
    every amp; and at amp 1 -- where the modulator's own amp, which also scales its training symbols and pilots, multiplies by
    one -- the same coded bytes through qam and ofdmmod in SYMBOLS mode give the very waveform of ofdmmod in BITS mode."""
    bits = mc.shape_args("n64", amp=1.0, order=4, in_mode=mc.BITS)
    syms = mc.shape_args("n64", amp=1.0, in_mode=mc.SYMBOLS)
    Nd, _, _, F, nbytes = mc.sizes(bits)
    n_sym = bits["n_data"] * Nd
    data = mc.rows(bits, 2, 3)
    assert api.qam_plan(4, n_sym) == (2, nbytes)
    for amp in (1.0, 0.37, 3.3e-3, 1e4 / 3):
        z = api.qam_plan(4, n_sym, amp=amp, data=data)
        a4 = F32(np.float64(F32(amp)) / np.sqrt(2.0))
        assert set(np.unique(_bits(z.view(F32)))) == set(_bits([a4, -a4]))
        assert np.array_equal(z.real < 0, np.unpackbits(data, axis=1)[:, 0:2 * n_sym:2] == 1)
        assert np.array_equal(z.imag < 0, np.unpackbits(data, axis=1)[:, 1:2 * n_sym:2] == 1)
    want = api.ofdmmod_plan(**bits, data=data, n_out=2 * F, start_step=F)
    got = api.ofdmmod_plan(**syms, data=api.qam_plan(4, n_sym, amp=1.0, data=data), n_out=2 * F, start_step=F)
    assert mc.same(got, want)


# ------------------------------------------------------------------------------------------------ the law, exactly
CASES = [(order, period, pk) for order in qc.ORDERS for period, pk in ((0, "none"), (52, "random"), (7, "reversal"), (0, "random"), (1, "none"))]


@pytest.mark.parametrize("order,period,pk", CASES)
def test_the_plan_is_the_law_operation_by_operation(api, order, period, pk):
    """Noise around the points at several scales: the plan's words equal the numpy restatement's, bit for bit."""
    n_rows, n_sym = 3, 301
    B = n_sym * qc.BPS[order]
    perm = qc.perm_of(pk, B, order)
    idx, clen, h = qc.csi_of(period, n_rows, order)
    for amp, noise, scale in ((1.0, 0.3, 1.0), (0.013, 0.05, 37.5), (811.0, 1.5, 2.0 ** -7), (1.0, 6.0, 1.0)):
        z = qc.noisy_symbols(order, n_rows, n_sym, amp, noise, seed=period)
        got = api.qam_plan(order, n_sym, amp, scale, perm, idx, clen, sym=z, csi=h)
        want = qc.law_numpy(z, order, amp, scale, perm, h, idx)
        assert got.shape == want.shape == (n_rows, B)
        assert np.array_equal(_bits(got), _bits(want)), (order, period, pk, amp)


@pytest.mark.parametrize("order", qc.ORDERS)
def test_plan_against_the_float64_reference(api, order):
    """|r - r_ref| <= 8 * 2^-24 * w * (D0 + D1), D0 and D1 the axis's own in float64; the reference tries all M points."""
    n_rows, n_sym, bps, m = 2, 257, qc.BPS[order], qc.axis_bits(order)
    perm = qc.perm_of("random", n_sym * bps, 40 + order)
    worst = 0.0
    for period in (0, 52):
        idx, clen, h = qc.csi_of(period, n_rows, order)
        for amp, noise, scale in ((1.0, 0.3, 1.0), (0.013, 0.05, 37.5), (811.0, 2.5, 0.01)):
            z = qc.noisy_symbols(order, n_rows, n_sym, amp, noise, seed=3)
            got = api.qam_plan(order, n_sym, amp, scale, perm, idx, clen, sym=z, csi=h).astype(np.float64)
            ref = synth.qam_reference(z, order, amp, scale, perm, h, idx)
            # the bar: per axis D0 + D1 over the levels, in float64
            lev = synth.qam_levels(order, amp).astype(np.float64)
            _, wbits = synth.qam_axis_words(m)
            w = np.full(z.shape, float(F32(scale)))
            if idx is not None:
                hh = h.astype(np.complex128)[:, idx[np.arange(n_sym) % idx.size]]
                w = w * (hh.real ** 2 + hh.imag ** 2)
            dsum = np.empty(z.shape + (bps,))
            for ax, y in enumerate((z.real, z.imag)[:1 if bps == 1 else 2]):
                e = (y.astype(np.float64)[..., None] - lev) ** 2
                for c in range(m):
                    one = wbits[:, c] == 1
                    dsum[..., ax * m + c] = e[..., one].min(axis=-1) + e[..., ~one].min(axis=-1)
            bar = (8 * 2.0 ** -24 * w[..., None] * dsum).reshape(n_rows, -1)
            sc = np.empty_like(bar)
            sc[:, perm] = bar
            ratio = float((np.abs(got - ref) / sc).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, (order, period, amp, ratio)
    print("qam order %d: worst |r - r_ref| is %.3f of the bar 8 * 2^-24 * w * (D0 + D1)" % (order, worst))


@pytest.mark.parametrize("order", qc.ORDERS)
def test_the_round_trip(api, order):
    """demap(map(bits)) at scale 1: r != 0 and (r < 0) == bit at every position, with a random perm; the floats land at
    perm[t] -- the row demapped without perm, scattered by perm, is the row demapped with it."""
    n_rows, n_sym = 3, 200
    bps, nbytes = api.qam_plan(order, n_sym)
    B = n_sym * bps
    perm = qc.perm_of("random", B, order)
    data = qc.coded_bytes(n_rows, nbytes, order)
    bits = np.unpackbits(data, axis=1)[:, :B]
    z = api.qam_plan(order, n_sym, 1.0, 1.0, perm, data=data)
    r = api.qam_plan(order, n_sym, 1.0, 1.0, perm, sym=z)
    assert (r != 0).all() and np.array_equal(r < 0, bits == 1)
    plain = api.qam_plan(order, n_sym, 1.0, 1.0, None, sym=z)
    assert np.array_equal(_bits(r[:, perm]), _bits(plain))
    # the mapper with perm reads coded bit perm[t] at position t: the unpermuted mapper on the gathered bits
    gathered = np.packbits(bits[:, perm], axis=1)
    assert np.array_equal(api.qam_plan(order, n_sym, 1.0, 1.0, None, data=gathered).view(np.uint32), z.view(np.uint32))


def test_the_exact_case(api):
    r = api.qam_plan(2, 1, amp=1.0, scale=1.0, sym=np.array([0.5 + 0j], np.complex64))
    assert r.shape == (1, 1) and _bits(r)[0, 0] == _bits([2.0])[0]
    r = api.qam_plan(2, 2, amp=1.0, scale=1.0, sym=np.array([0.5 + 9j, -0.5 - 3j], np.complex64))        # Q is ignored
    assert np.array_equal(r, [[2.0, -2.0]])
    z = api.qam_plan(2, 8, data=np.array([0b01100000], np.uint8))
    assert np.array_equal(_bits(z.view(F32)).ravel(), _bits(np.array([1, 0, -1, 0, -1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0], F32)))       # Q is +0


def test_rows_strides_and_unaligned_host_buffers(api, L):
    """Rows lie at their strides; what lies between rows is neither read into the answer nor written; any byte alignment."""
    from simplefe_amd import lib
    order, n_sym, n_rows = 64, 11, 3
    bps, nbytes = api.qam_plan(order, n_sym)
    B = n_sym * bps
    idx, clen, h = qc.csi_of(52, n_rows, 1)
    z = qc.noisy_symbols(order, n_rows, n_sym, seed=8)
    want = api.qam_plan(order, n_sym, csi_index=idx, csi_len=clen, sym=z, csi=h)
    zs, hs, os_ = n_sym + 3, clen + 2, B + 5
    raw_z, raw_h = np.full(8 * n_rows * zs + 1, 0xEE, np.uint8), np.full(8 * n_rows * hs + 3, 0xEE, np.uint8)
    for r in range(n_rows):
        raw_z[1 + 8 * r * zs:][:8 * n_sym] = z[r].view(np.uint8)
        raw_h[3 + 8 * r * hs:][:8 * clen] = h[r].view(np.uint8)
    raw_o = np.full(4 * n_rows * os_ + 2, 0x5A, np.uint8)
    head, _alive = _shape(order, 1.0, 1.0, n_sym, None, idx.size, clen, idx)
    assert L.sfe_dsp_qam_plan(*head, lib.QAM_DEMAP, raw_z.ctypes.data + 1, zs, raw_h.ctypes.data + 3, hs, n_rows, raw_o.ctypes.data + 2, os_,
                              None, None) == lib.SFE_OK
    body = raw_o[2:].reshape(n_rows, 4 * os_)
    assert np.array_equal(body[:, :4 * B].copy().view(F32), want) and (body[:, 4 * B:] == 0x5A).all() and (raw_o[:2] == 0x5A).all()


# ------------------------------------------------------------------------------------------------ the law header, stand-alone
def test_the_law_under_the_sanitizers(tmp_path):
    """tests/host/test_qam_law.cpp, a stand-alone program with its own main, built with the host compiler and
    -fsanitize=address,undefined: the axis words, the kernel's form of an axis against the statement, rows from heap blocks of
    exactly the contract's sizes against a brute-force double loop."""
    exe = str(tmp_path / "qam_law")
    r = subprocess.run(["g++", "-O1", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-std=c++17", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", os.path.join(ROOT, "tests/host/test_qam_law.cpp"), "-o", exe], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "qam law ok: " in r.stdout, r.stdout + r.stderr


# ------------------------------------------------------------------------------------------------ the chain
def test_the_chain_on_the_cpu_needs_the_channel_weighting(api):
    """payload -> ldpc_plan (encode, n = 648) -> qam_plan (map, 16-QAM, random perm) -> ofdmmod_plan (SYMBOLS, N = 64) -> the
    two-tap channel 1, 0.9 exp(0.4j) at delay 2 and fixed-seed noise -> ofdm_plan (ZF, chan) -> qam_plan (demap, CSI) ->
    ldpc_plan (decode).  The noise level chosen: a standard deviation of 0.016 per component (qam_cases.CHAIN_NOISE) on a
    waveform of RMS 0.11 -- between 0.008, from where on the unweighted demapper leaves a word unconverged, and 0.024, up to
    where the weighted one still converges every word (two iterations each at 0.016).  Every word converges (status 0) to its
    payload with the weighting; the same symbols demapped without it leave at least one word unconverged or wrong."""
    from simplefe_amd import lib
    o = qc.chain_on_the_cpu(api, lib)          # asserts both halves
    want = lc.payload_bits_only("B", o["pay"])
    assert not o["dec"][2].any() and np.array_equal(o["dec"][0], want)
    print("chain: noise %.3g, weakest data bin |H|^2 / mean %.2e, iterations %s with CSI; without: status %s, words lost %s"
          % (qc.CHAIN_NOISE, o["min_h2"], o["dec"][1][:, 0].tolist(), o["dec_flat"][2].tolist(), o["bad_flat"]))
    assert o["bad_flat"]
    # the channel really has a null among the data bins, and the received symbols really are 16-QAM at the mapper's amp
    assert o["min_h2"] < 0.01
    assert o["sym"].shape == (4, 162) and o["llr"].shape == (4, 648)
    hard = (o["llr"] < 0)
    code_bits = np.unpackbits(o["code"], axis=1)[:, :648]
    assert 0 < int((hard != code_bits).sum()) < 648          # the decoder had wrong decisions to repair
