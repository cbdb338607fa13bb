"""The 2-(G)FSK burst modem (sfe_dsp_fsk_*) without a GPU: the C ABI's declarations and exports, the build lists, the kernels'
resources, the refusals of the plan and of create, fsk_cis, both plan directions against a restatement of the law in numpy
(uint32 phases, float32 operations one at a time: bit equality) and against the float64 references of simplefe_amd/synth.py
(independent of the header), the exact case, the round trips, the statuses, the chain through the plans, and the law header
under the sanitizers.

The bars against float64 are derived, not measured, and the worst ratio to each is printed.  Modulator: |y - y_ref| <= amp *
(2 pi 0.5 n_taps N 2^-32 + 2 * 2^-23) -- each of the N symbols' n_taps integer increments is off by at most half a unit of
2^-32 turns, then fsk_cis and one product.  Demodulator, with dv = 3 ulp(pi) = 7.15e-7 rad the FM detector's own bar
(DESIGN.md 4.19), M1 = sum |m|, A = sum |e|, Umax = pi M1, d = log2 of the padded preamble length and u24 = 2^-24:
    du    = M1 (dv + n_mf u24 pi)                                          n_mf fmaf roundings
    dSe   = A du + (d + 1) u24 A Umax,   dS1 = Lp du + d u24 Lp Umax       the products, then d levels of the tree
    dnum  = Lp dSe + |se| dS1 + 2 u24 Lp Umax (A + |se|)
    ddev  = dnum / den + 2 u24 dev                                         one division; den's own rounding
    ddc   = (dS1 + |se| ddev + 3 u24 (|S1| + |dev se|)) / Lp,   df = ddc / (2 pi) + u24 |f|
    dsoft = scale ((du + ddc) / dev + |u - dc| ddev / dev^2 + 3 u24 |w|)"""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import fsk_cases as fc
import reed_cases as rc
from simplefe_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "sfe_dsp.h")
FSK_FUNCS = ("sfe_dsp_fsk_plan", "sfe_dsp_fsk_create", "sfe_dsp_fsk_set_input_format", "sfe_dsp_fsk_mod_stream", "sfe_dsp_fsk_demod_stream",
             "sfe_dsp_fsk_destroy")
F32 = np.float32
U24 = 2.0 ** -24


@pytest.fixture(scope="module")
def L():
    from simplefe_amd import lib
    return lib.load()


@pytest.fixture(scope="module")
def api():
    from simplefe_amd import api as a
    return a


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------ ABI and build lists
def test_header_declares_fsk_abi_and_library_exports_it(L):
    from simplefe_amd import lib
    hdr = open(HDR).read()
    assert set(re.findall(r"\b(sfe_dsp_fsk_[a-z0-9_]+)\s*\(", hdr)) == set(FSK_FUNCS)
    assert {n for n in lib.SIGNATURES if n.startswith("sfe_dsp_fsk_")} == set(FSK_FUNCS)
    for name in FSK_FUNCS:
        assert hasattr(L, name), name
    for name, v in (("SFE_FSK_MOD", 0), ("SFE_FSK_DEMOD", 1)):
        assert re.search(r"#define %s %d\b" % (name, v), hdr), name
    assert (lib.FSK_MOD, lib.FSK_DEMOD) == (0, 1)


def test_fsk_sources_are_in_the_build_lists():
    from simplefe_amd import build
    assert "fsk.hip" in build.EXACT_SOURCES and "api_fsk.hip" in build.HOST_SOURCES
    assert build.KERNEL_FILES["fsk"][:4] == ("fsk.hip", "fsk.h", "fsk_law.h", "polar_law.h") and "mod.h" in build.KERNEL_FILES["fsk"]
    assert build.SCRATCH_FREE["fsk.hip"] == "FSK-modem"
    cm = open(os.path.join(ROOT, "CMakeLists.txt")).read()
    assert re.search(r"set\(SFE_EXACT_SOURCES [^)]*\bfsk\.hip\b", cm)
    for f in build.KERNEL_FILES["fsk"] + ("api_fsk.hip",):
        assert os.path.exists(os.path.join(build.CSRC, f)), f
    text = {f: open(os.path.join(build.CSRC, f)).read() for f in ("fsk.hip", "api_fsk.hip", "fsk.h", "fsk_law.h", "mod.hip")}
    assert '#include "fsk.h"' in text["fsk.hip"] and '#include "fsk.h"' in text["api_fsk.hip"] and '#include "fsk_law.h"' in text["fsk.h"]
    # the discriminator is polar's, included and not copied; the store path is mod's, shared through mod.h
    assert '#include "polar_law.h"' in text["fsk_law.h"] and "polar_sample<POLAR_FM>" in text["fsk_law.h"] and "POLAR_C0" not in text["fsk_law.h"]
    assert '#include "mod.h"' in text["fsk.hip"] and "mod_store_pair<TX10>" in text["fsk.hip"] and "mod_store_pair<TX10>" in text["mod.hip"]
    assert text["fsk_law.h"].count("#pragma clang fp contract(off)") >= 9          # every function that computes
    assert "4-level" in text["fsk_law.h"]


def test_fsk_kernels_use_no_scratch_and_the_lds_they_state():
    """fsk.h states the LDS: the modulator's C table, levels, prefix sums and four counts, 21056 bytes; the demodulator's two
    trees and two candidate tables, 33824 bytes, and one flag word more on cf32 input."""
    from simplefe_amd import build
    build.build_lib()
    res = json.load(open(os.path.join(build.HERE, "build", "fsk.hip.resources.json")))
    names = {re.search(r"(fsk_\w+_kernel<\w+>)", k).group(1): v for k, v in res.items()}
    assert set(names) == {"fsk_mod_kernel<false>", "fsk_mod_kernel<true>", "fsk_demod_kernel<false>", "fsk_demod_kernel<true>"}
    taps, syms = 64 * 64, 1024 // 2 + 64 + 2
    r16 = lambda b: (b + 15) // 16 * 16
    want = {"fsk_mod_kernel<false>": r16(4 * (taps + 1)) + r16(4 * syms) + r16(4 * (syms + 1)) + 16,
            "fsk_demod_kernel<true>": 2 * 4096 * 4 + 2 * 132 * 4}
    want["fsk_mod_kernel<true>"] = want["fsk_mod_kernel<false>"]
    want["fsk_demod_kernel<false>"] = want["fsk_demod_kernel<true>"] + 4
    assert want["fsk_mod_kernel<true>"] == 21056 and want["fsk_demod_kernel<false>"] == 33828
    for k, v in names.items():
        assert v.get("ScratchSize", 1) == 0 and v.get("VGPRs Spill", 0) == 0 and v.get("SGPRs Spill", 0) == 0, (k, v)
        assert v.get("LDS Size", -1) == want[k], (k, v)
    print("fsk kernels: " + "; ".join("%s %d VGPRs %d SGPRs" % (k, v["VGPRs"], v["TotalSGPRs"]) for k, v in sorted(names.items())))


# ------------------------------------------------------------------------------------------------ refusals
def _head(kw):
    g, p, m = np.ascontiguousarray(kw["pulse"], F32), np.ascontiguousarray(kw["pre"], np.uint8), np.ascontiguousarray(kw["mf"], F32)
    return (kw["sps"], g.ctypes.data if g.size else None, g.size, kw["h"], kw["amp"], p.ctypes.data if p.size else None, p.size, kw["n_bits"],
            m.ctypes.data if m.size else None, m.size, kw["delay"], kw["rng"], kw["scale"], kw["min_gate"], kw["out_fmt"]), (g, p, m)


BASE = fc.shape(4, 0.5, 3)
NAN, INF = float("nan"), float("inf")
REFUSALS = [("sps 1", dict(sps=1)), ("sps 65", dict(sps=65)), ("no taps", dict(pulse=np.zeros(0, F32))), ("n_taps 64 sps + 1", dict(pulse=np.full(257, 1e-3, F32))),
            ("a NaN in the pulse", dict(pulse=np.array([0.2, NAN, 0.2, 0.2], F32))), ("h 0", dict(h=0.0)), ("a NaN h", dict(h=NAN)), ("an infinite h", dict(h=INF)),
            ("amp 0", dict(amp=0.0)), ("an infinite amp", dict(amp=INF)), ("one preamble bit", dict(pre=[1])), ("1025 preamble bits", dict(pre=[0, 1] * 512 + [1])),
            ("a preamble bit of 2", dict(pre=[0, 1, 2, 0])), ("n_bits 0", dict(n_bits=0)), ("n_bits 32769", dict(n_bits=32769)),
            ("no matched filter", dict(mf=np.zeros(0, F32))), ("n_mf 257", dict(mf=np.full(257, 1.0, F32))), ("an infinite matched-filter value", dict(mf=np.array([1, INF], F32))),
            ("a matched filter of sum 0", dict(mf=np.array([1, -1], F32))), ("delay 0", dict(delay=0)), ("delay 2^20 + 1", dict(delay=(1 << 20) + 1)),
            ("range -1", dict(rng=-1)), ("range 65", dict(rng=65)), ("scale 0", dict(scale=0.0)), ("a NaN scale", dict(scale=NAN)), ("a NaN min_gate", dict(min_gate=NAN)),
            ("an infinite min_gate", dict(min_gate=INF)), ("out_fmt U8", dict(out_fmt=1)), ("a pulse of sum 0", dict(pulse=np.array([0.25, -0.25, 0.25, -0.25], F32))),
            ("a negative pulse", dict(pulse=np.full(4, -0.25, F32))), ("a quarter turn a sample", dict(pulse=np.full(4, 1.0, F32))),
            ("a residue that sums to a quarter turn", dict(pulse=np.full(8, 0.5, F32))),
            ("a preamble without spread", dict(pulse=np.full(4, 0.25, F32), pre=[0] * 8, delay=1))]


@pytest.mark.parametrize("why,kw", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_plan_and_create_refuse_before_the_device_is_touched(L, why, kw):
    from simplefe_amd import lib
    head, _alive = _head(dict(BASE, **kw))
    N, F, den = C.c_int(9), C.c_int(9), C.c_float(9)
    assert L.sfe_dsp_fsk_plan(*head, lib.FSK_MOD, None, 0, None, None, 0, 0, 0, None, 0, None, None, None, C.byref(N), C.byref(F), None,
                              C.byref(den)) == lib.SFE_EINVAL, why
    assert L.sfe_dsp_last_error().startswith(b"fsk: "), (why, L.sfe_dsp_last_error())
    assert N.value == 0 and F.value == 0 and den.value == 0
    h = C.c_void_p()
    assert L.sfe_dsp_fsk_create(*head, 1, 0, C.byref(h)) == lib.SFE_EINVAL, why
    assert L.sfe_dsp_last_error().startswith(b"fsk: ") and not h.value, (why, L.sfe_dsp_last_error())


def test_create_refuses_no_streams_and_the_plan_its_buffers(L, api):
    from simplefe_amd import lib
    head, _alive = _head(BASE)
    h = C.c_void_p()
    assert L.sfe_dsp_fsk_create(*head, 0, 0, C.byref(h)) == lib.SFE_EINVAL and L.sfe_dsp_last_error().startswith(b"fsk: ")
    N, F, e, den = api.fsk_plan(**BASE)
    assert (N, F) == (88, (88 + 3 - 1) * 4 + 1) and e.size == 24 and den > 0
    data, out = fc.payload(64, 2, 1), np.full(2 * F, 7 + 7j, np.complex64)

    def plan(direction=lib.FSK_MOD, pi=data.ctypes.data, ilen=8, nb=2, base=0, step=F, po=out.ctypes.data, n_out=2 * F):
        return L.sfe_dsp_fsk_plan(*head, direction, pi, ilen, None, None, nb, base, step, po, n_out, None, None, None, None, None, None, None)

    assert plan(ilen=7) == lib.SFE_ERANGE and L.sfe_dsp_last_error().startswith(b"fsk: ")
    for why, rc_ in (("direction 2", plan(direction=2)), ("null bytes", plan(pi=None)), ("a negative start_base", plan(base=-1)),
                     ("frames that overlap", plan(step=F - 1)), ("a frame behind the stream", plan(base=1)), ("n_out 2^31", plan(n_out=1 << 31)),
                     ("demod without soft values", plan(direction=lib.FSK_DEMOD, po=None))):
        assert rc_ == lib.SFE_EINVAL and L.sfe_dsp_last_error().startswith(b"fsk: "), why
    assert (out == np.complex64(7 + 7j)).all()
    assert plan() == lib.SFE_OK and not (out == np.complex64(7 + 7j)).any()
    with pytest.raises(lib.SfeError):
        api.fsk_plan(**dict(BASE, out_fmt=lib.FMT_TX10), data=data, n_out=2 * F + 1, start_step=F)         # an odd n_out under TX10


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present: create succeeds there")
def test_create_without_gpu_is_enodev():
    from simplefe_amd import api, lib
    with pytest.raises(lib.SfeError) as e:
        api.Fsk(**{k: v for k, v in BASE.items()})
    assert e.value.code == lib.SFE_ENODEV


def test_null_handles_are_refused(L):
    from simplefe_amd import lib
    k = C.c_size_t(5)
    assert L.sfe_dsp_fsk_mod_stream(None, None, 8, 1, 0, 0, None, 400, C.byref(k), None) == lib.SFE_EINVAL
    assert L.sfe_dsp_last_error().startswith(b"fsk_mod_stream: ") and k.value == 0
    k = C.c_size_t(5)
    assert L.sfe_dsp_fsk_demod_stream(None, None, 400, 400, None, 1, None, 1, 1, 0, 0, None, 64, None, 8, None, None, 1, C.byref(k), None) == lib.SFE_EINVAL
    assert L.sfe_dsp_last_error().startswith(b"fsk_demod_stream: ") and k.value == 0
    assert L.sfe_dsp_fsk_set_input_format(None, 0) == lib.SFE_EINVAL
    assert L.sfe_dsp_fsk_destroy(None) == lib.SFE_OK


# ------------------------------------------------------------------------------------------------ fsk_cis
def test_cis_is_exact_at_the_quadrants_and_within_2_ulp():
    """The numpy restatement of fsk_cis (held to the plan's words by the mod tests below): exact at the four quadrant phases;
    within 2 ulp(1) = 2.39e-7 of float64 on every 4099th phase and on the +-4096 neighbours of the eight multiples of 2^29."""
    c, s = fc.cis_numpy(np.arange(4, dtype=np.uint64) << 30)
    assert np.array_equal(np.abs(c), [1, 0, 1, 0]) and np.array_equal(np.abs(s), [0, 1, 0, 1])
    assert c[0] == 1 and s[1] == 1 and c[2] == -1 and s[3] == -1
    p = np.concatenate([np.arange(0, 1 << 32, 4099, dtype=np.uint64)] +
                       [((np.uint64(m) << 29) + np.arange(-4096, 4097).astype(np.int64)).astype(np.uint64) & 0xFFFFFFFF for m in range(8)])
    c, s = fc.cis_numpy(p)
    a = 2 * np.pi * p.astype(np.float64) / 2.0 ** 32
    worst = max(float(np.abs(c - np.cos(a)).max()), float(np.abs(s - np.sin(a)).max()))
    print("fsk_cis: worst error %.4g of the bar %.4g on %d phases" % (worst, 2 * 2.0 ** -23, p.size))
    assert worst <= 2 * 2.0 ** -23


# ------------------------------------------------------------------------------------------------ the modulator
@pytest.mark.parametrize("p", fc.PROBES, ids=fc.PROBE_IDS)
def test_mod_plan_is_the_integer_law_and_near_the_float64_reference(api, p):
    worst = 0.0
    for amp, seed in ((1.0, 0), (0.37, 1), (811.0, 2)):
        kw = fc.probe(p, amp=amp)
        N, F, _, _ = api.fsk_plan(**kw)
        data = fc.payload(64, 3, seed)
        y = api.fsk_plan(**kw, data=data, n_out=3 * F + 10, start_base=7, start_step=F + 1)
        eps = 2 * np.pi * 0.5 * kw["pulse"].size * N * 2.0 ** -32 + 2 * 2.0 ** -23
        for b in range(3):
            got = y[7 + b * (F + 1):][:F]
            assert np.array_equal(_bits(got.view(F32)), _bits(fc.mod_numpy(kw, data[b]).view(F32))), (p, amp, b)
            ref = synth.fsk_reference_mod(kw["pre"], np.unpackbits(data[b])[:64], kw["pulse"], kw["h"], kw["sps"], amp)
            assert ref.size == F
            ratio = float(np.abs(got.astype(np.complex128) - ref).max() / (float(F32(amp)) * eps))
            worst = max(worst, ratio)
            assert ratio <= 1.0, (p, amp, b, ratio)
        outside = np.ones(y.size, bool)
        for b in range(3):
            outside[7 + b * (F + 1):][:F] = False
        assert not y[outside].view(np.uint32).any()             # a sample in no frame is +0
    print("fsk mod %s: worst |y - y_ref| is %.3f of the bar amp * (2 pi 0.5 n_taps N 2^-32 + 2^-22)" % (p, worst))


def test_tx10_is_the_converters_bytes_of_the_f32_stream(api):
    from simplefe_amd import lib
    kw = fc.probe(fc.PROBES[0], amp=0.8)
    N, F, _, _ = api.fsk_plan(**kw)
    data = fc.payload(64, 2, 5)
    place = dict(n_out=2 * F + 12, start_base=3, start_step=F + 3)              # frames start mid-group
    y = api.fsk_plan(**kw, data=data, **place)
    tx = api.fsk_plan(**dict(kw, out_fmt=lib.FMT_TX10), data=data, **place)
    assert np.array_equal(tx, synth.tx10_pack(y))


def test_the_exact_case_msk(api):
    """A rectangular pulse of n_taps = sps = 8, g = 1/8, h = 0.5: every G is 2^27, a symbol turns the phase by exactly a
    quarter.  The sample at every symbol boundary is exactly (+-amp, +-0) or (+-0, +-amp); |y|^2 is within 4 ulp of amp^2."""
    amp = F32(0.7)
    kw = fc.shape(8, n_rect=8, amp=amp)
    N, F, _, _ = api.fsk_plan(**kw)
    data = fc.payload(64, 1, 9)
    y = api.fsk_plan(**kw, data=data, n_out=F)
    assert F == N * 8 + 1
    b = y[::8]
    assert b.size == N + 1
    on_axis = ((np.abs(b.real) == amp) & (b.imag == 0)) | ((np.abs(b.imag) == amp) & (b.real == 0))
    assert on_axis.all()
    lev = fc.phases_numpy(kw, data[0])[::8]
    assert np.array_equal(lev & ((1 << 30) - 1), np.zeros(N + 1, np.uint64))
    p2 = y.real.astype(np.float64) ** 2 + y.imag.astype(np.float64) ** 2
    a2 = float(amp) ** 2
    assert np.abs(p2 / a2 - 1).max() <= 4 * 2.0 ** -23
    # F includes the final sample: the last symbol's quarter turn is complete inside the frame
    bits = np.concatenate([kw["pre"], np.unpackbits(data[0])[:64]])
    total = int((1 - 2 * bits.astype(np.int64)).sum()) % 4
    want = [(1, 0), (0, 1), (-1, 0), (0, -1)][total]
    assert (y[-1].real, y[-1].imag) == (want[0] * amp, want[1] * amp)
    assert y[-1] != y[-2]


def test_a_frame_depends_on_its_bytes_and_pad_bits_are_ignored(api):
    kw = fc.probe(fc.PROBES[2], n_bits=61)
    N, F, _, _ = api.fsk_plan(**kw)
    data = fc.payload(61, 2, 4)
    other = data.copy()
    other[:, -1] ^= 0x07                                        # the three pad bits
    a = api.fsk_plan(**kw, data=data, n_out=2 * F, start_step=F)
    b = api.fsk_plan(**kw, data=other[::-1], n_out=2 * F + 50, start_base=13, start_step=F + 30)
    assert np.array_equal(_bits(a[:F].view(F32)), _bits(b[13 + F + 30:][:F].view(F32)))
    assert np.array_equal(_bits(a[F:].view(F32)), _bits(b[13:][:F].view(F32)))


# ------------------------------------------------------------------------------------------------ the demodulator
def _bars(kw, e, se, see, den, rec, S1, u_data):
    m = np.abs(np.asarray(kw["mf"], np.float64))
    Lp, n_mf = e.size, m.size
    M1, A, d = m.sum(), np.abs(e).sum(), int(np.ceil(np.log2(Lp)))
    dv, Umax = 3 * 2.0 ** -22, np.pi * m.sum()
    tau, f, dev, q = (float(v) for v in rec[:4])
    dc = f * 2 * np.pi
    du = M1 * (dv + n_mf * U24 * np.pi)
    dSe, dS1 = A * du + (d + 1) * U24 * A * Umax, Lp * du + d * U24 * Lp * Umax
    dnum = Lp * dSe + abs(se) * dS1 + 2 * U24 * Lp * Umax * (A + abs(se))
    ddev = dnum / den + 2 * U24 * dev
    ddc = (dS1 + abs(se) * ddev + 3 * U24 * (abs(S1) + abs(dev * se))) / Lp
    df = ddc / (2 * np.pi) + U24 * abs(f)
    w = (u_data - dc) / dev
    dsoft = float(F32(kw["scale"])) * ((du + ddc) / dev + np.abs(u_data - dc) * ddev / dev ** 2 + 3 * U24 * np.abs(w))
    return df, ddev, dsoft


@pytest.mark.parametrize("p", fc.PROBES, ids=fc.PROBE_IDS)
def test_demod_plan_is_the_law_and_near_the_float64_reference(api, p):
    worst = 0.0
    for scale, seed, late in ((1.0, 0, 0), (4.0, 1, 1), (0.25, 2, -1)):
        kw = fc.probe(p, scale=scale)
        N, F, e, den = api.fsk_plan(**kw)
        e2, se, see, den2 = fc.expected_numpy(kw)
        assert np.array_equal(_bits(e), _bits(e2)) and F32(den) == den2
        data = fc.payload(64, 1, seed)
        x = fc.channel(api.fsk_plan(**kw, data=data, n_out=F), F + 200, 37, seed=seed).astype(np.complex64)
        o = 37 + late
        soft, by, rec, st = api.fsk_plan(**kw, x=x, start_base=o)
        s2, b2, r2, st2 = fc.demod_numpy(kw, x, o)
        assert st[0] == st2 == 0
        assert np.array_equal(_bits(soft[0]), _bits(s2)) and np.array_equal(by[0], b2) and np.array_equal(_bits(rec[0]), _bits(r2)), (p, scale)
        assert not rec[0, 4:].view(np.uint32).any()
        tau, f, dev, q, ref = synth.fsk_reference_demod(x, o, kw["pre"], 64, kw["pulse"], kw["sps"], kw["mf"], kw["delay"], kw["rng"], scale)
        assert rec[0, 0] == tau and abs(tau + late) <= 1                # (noise may move the flat top of sps 10 by a sample)
        dc = f * 2 * np.pi
        u_data = ref / float(F32(scale)) * dev + dc
        S1 = 24 * dc + dev * float(se)
        df, ddev, dsoft = _bars(kw, e.astype(np.float64), float(se), float(see), float(den), rec[0], S1, u_data)
        ratios = (abs(float(rec[0, 1]) - f) / df, abs(float(rec[0, 2]) - dev) / ddev, float((np.abs(soft[0] - ref) / dsoft).max()))
        worst = max(worst, *ratios)
        assert max(ratios) <= 1.0, (p, scale, ratios)
        assert abs(float(rec[0, 3]) - q) <= 1e-4 * max(q, 1e-3)
    print("fsk demod %s: worst ratio of |f - f_ref|, |dev - dev_ref|, |soft - soft_ref| to their bars: %.4f" % (p, worst))


@pytest.mark.parametrize("p", fc.PROBES, ids=fc.PROBE_IDS)
def test_round_trips_return_every_bit(api, p):
    """Preamble 0101... (16 bits) + 00110100, 64 data bits, the frame at offset 37 of a zero stream, a carrier offset of 0.01
    turns per sample, a phase of 1 rad, complex white noise at 20 dB, seeds 0 - 19: every bit returns; f within 10 % of 0.01 and
    dev within 10 % of pi h / sps."""
    kw = fc.probe(p)
    N, F, _, _ = api.fsk_plan(**kw)
    errors, fs, devs = 0, [], []
    for seed in range(20):
        data = fc.payload(64, 1, 100 + seed)
        x = fc.channel(api.fsk_plan(**kw, data=data, n_out=F), F + 200, 37, f=0.01, phase=1.0, snr_db=20.0, seed=seed).astype(np.complex64)
        soft, by, rec, st = api.fsk_plan(**kw, x=x, start_base=37)
        assert st[0] == 0
        errors += int((np.unpackbits(by[0]) != np.unpackbits(data[0])).sum())
        assert np.array_equal(soft[0] < 0, np.unpackbits(data[0]) == 1)
        fs.append(float(rec[0, 1]))
        devs.append(float(rec[0, 2]))
    want_dev = np.pi * 0.5 / kw["sps"]
    print("fsk round trip %s: %d errors in 1280 bits; f in [%.5f, %.5f]; dev / (pi h / sps) in [%.4f, %.4f]"
          % (p, errors, min(fs), max(fs), min(devs) / want_dev, max(devs) / want_dev))
    assert errors == 0
    assert max(abs(f - 0.01) for f in fs) <= 0.1 * 0.01
    assert max(abs(d - want_dev) for d in devs) <= 0.1 * want_dev


def test_statuses_and_their_fill(api):
    kw = fc.probe(fc.PROBES[0], min_gate=0.5)
    N, F, _, _ = api.fsk_plan(**kw)
    data = fc.payload_clean(64, 1, 3)
    x = fc.channel(api.fsk_plan(**kw, data=data, n_out=F), F + 100, 37, seed=3).astype(np.complex64)
    bad = x.copy()
    bad[37 + 200] = np.nan
    lo = kw["delay"] - kw["rng"] - 1
    cases = [(x, 37, None, 0), (bad, 37, None, 1), (x, 37, [0.25], 2), (x, 37, [np.nan], 2), (x, -lo - 1, None, 3), (x, -lo, None, 0),
             (x, 37 + 101, None, 3), (x, 1 << 40, None, 3), (bad, 37, [0.0], 2)]
    for xx, o, gate, want in cases:
        soft, by, rec, st = api.fsk_plan(**kw, x=xx, start_base=o, gate=gate)
        assert st[0] == want, (o, gate, st)
        if want:
            assert not soft.view(np.uint32).any() and not by.any()
            assert np.array_equal(rec.view(np.uint32)[0, :4], [0x7FC00000] * 4) and not rec.view(np.uint32)[0, 4:].any()
    soft, by, rec, st = api.fsk_plan(**kw, x=x, start_base=37)
    assert np.array_equal(by[0], data[0])
    # the reach's last sample: one sample fewer in the stream and the burst is out of range
    hi = 37 + kw["delay"] + kw["rng"] + (N - 1) * kw["sps"] + kw["mf"].size
    assert api.fsk_plan(**kw, x=x[:hi], start_base=37)[3][0] == 0 and api.fsk_plan(**kw, x=x[:hi - 1], start_base=37)[3][0] == 3


def test_the_chain_through_the_plans(api):
    """payload -> reed_plan (encode, shape C: 96 -> 120 bytes) -> fsk_plan (mod) -> a float64 channel (offset, phase, noise at
    9 dB) -> fsk_plan (demod, hard bytes) -> reed_plan (decode) -> the payload.  The noise level chosen: between 10 dB, down to
    where the discriminator makes no error on these frames, and 8 dB, where its clicks overwhelm the code (t = 4 bytes a
    codeword); at 9 dB the decoder has wrong bytes to repair and repairs them all."""
    shape = rc.SHAPES["C"]
    pay_bytes, frame_bytes, _ = rc.sizes(shape)
    pay = np.random.default_rng(12).integers(0, 256, (3, pay_bytes), dtype=np.uint8)
    frames = api.reed_plan(*shape, data=pay, encode=True)
    assert frames.shape == (3, frame_bytes)
    kw = fc.shape(4, 0.5, 3, n_bits=8 * frame_bytes)
    N, F, _, _ = api.fsk_plan(**kw)
    step = F + 40
    y = api.fsk_plan(**kw, data=frames, n_out=3 * step + 100, start_base=50, start_step=step)
    x = fc.channel(y, y.size, 0, f=0.006, phase=2.0, snr_db=9.0, seed=5).astype(np.complex64)
    soft, by, rec, st = api.fsk_plan(**kw, x=x, n_bursts=3, start_base=50, start_step=step)
    assert not st.any()
    wrong = int((np.unpackbits(by, axis=1) != np.unpackbits(frames, axis=1)).sum())
    out, rrec, rst = api.reed_plan(*shape, data=by)
    print("chain: %d channel bit errors in %d, Reed-Solomon corrected %s bytes" % (wrong, 3 * 8 * frame_bytes, rrec[:, 0].tolist()))
    assert wrong > 0 and not rst.any() and np.array_equal(out, pay)


# ------------------------------------------------------------------------------------------------ the law header, stand-alone
def test_the_law_under_the_sanitizers(tmp_path):
    """tests/host/test_fsk_law.cpp, a stand-alone program with its own main, built with the host compiler and
    -fsanitize=address,undefined: the cis words, the tile form of P[i] against the defining sum, the tree against its
    statement, every heap buffer exactly the contract's size."""
    exe = str(tmp_path / "fsk_law")
    r = subprocess.run(["g++", "-O1", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-std=c++17", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", os.path.join(ROOT, "tests/host/test_fsk_law.cpp"), "-o", exe], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "fsk law ok: " in r.stdout, r.stdout + r.stderr
