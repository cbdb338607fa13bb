"""The OFDM burst receiver (sfe_dsp_ofdm_*) without a GPU: the C ABI's declarations and exports, the build lists, the
host-only planner -- its refusals, its float64 law against synth.ofdm_reference (numpy on np.fft, written apart from it),
what it recovers from noiseless multipath bursts, the exact case, and statuses 1, 2 and 3 each from its own cause -- and
the no-GPU refusal of create."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ofdm_cases as oc
from simplefe_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "sfe_dsp.h")
OFDM_FUNCS = ("sfe_dsp_ofdm_plan", "sfe_dsp_ofdm_create", "sfe_dsp_ofdm_set_input_format", "sfe_dsp_ofdm_process_stream", "sfe_dsp_ofdm_destroy")
F32 = np.float32
QNAN_REC = np.array([np.nan] * 6 + [0, 0], F32)


@pytest.fixture(scope="module")
def api():
    from simplefe_amd import api as a
    return a


@pytest.fixture(scope="module")
def lib():
    from simplefe_amd import lib as l
    return l


def _bits(y):
    return np.ascontiguousarray(y).view(np.uint32)


def test_header_declares_ofdm_abi_and_library_exports_it(lib):
    L = lib.load()
    text = open(HDR).read()
    declared = set(re.findall(r"\b(sfe_dsp_ofdm_[a-z0-9_]+)\s*\(", text))
    assert declared == set(OFDM_FUNCS)
    assert re.search(r"#define SFE_OFDM_OUT_ZF 0\b", text) and re.search(r"#define SFE_OFDM_OUT_MRC 1\b", text)
    for name in OFDM_FUNCS:
        assert hasattr(L, name), name
        assert name in lib.SIGNATURES, name
    assert (lib.OFDM_OUT_ZF, lib.OFDM_OUT_MRC) == (0, 1)
    assert (lib.OFDM_OK, lib.OFDM_NO_ESTIMATE, lib.OFDM_GATED, lib.OFDM_OUT_OF_RANGE) == (0, 1, 2, 3)


def test_build_lists_name_the_files():
    from simplefe_amd import build
    assert "ofdm.hip" in build.EXACT_SOURCES and "api_ofdm.hip" in build.HOST_SOURCES
    assert build.KERNEL_FILES["ofdm"] == ("ofdm.hip", "ofdm.h", "fft16.h", "common.h")
    assert "ofdm.hip" in build.SCRATCH_FREE
    for f in ("ofdm.hip", "ofdm.h", "api_ofdm.hip"):
        assert os.path.exists(os.path.join(build.CSRC, f))
    cm = open(os.path.join(ROOT, "CMakeLists.txt")).read()
    assert re.search(r"set\(SFE_EXACT_SOURCES [^)]*\bofdm\.hip\b", cm)
    assert len(build.csrc_hash("ofdm")) == 64


def _good():
    """A small valid shape as keyword arguments: N = 64, cp = 8, two pilots."""
    kind = np.zeros(64, np.uint8)
    kind[1:20] = 1
    kind[[5, 12]] = 2
    return dict(n_fft=64, cp=8, advance=2, n_train=1, n_data=2, kind=kind, train=np.ones(64, np.complex64), pilot=np.ones(64, np.complex64),
                pilot_sign=np.array([1, -1], np.int8), cfo_mode=1, cfo_skip=3, out_mode=0, min_gate=0.0)


def _refused(api, lib, **change):
    """Plan and create both refuse with an "ofdm: " message; create does so before it looks for a device."""
    a = dict(_good(), **change)
    for call in (lambda: api.ofdm_plan(**a), lambda: api.Ofdm(**a)):
        with pytest.raises(lib.SfeError) as e:
            call()
        assert e.value.code == lib.SFE_EINVAL and "error -1: ofdm: " in str(e.value), str(e.value)
    return str(e.value)


def _table(n, k, v, dtype=np.complex64):
    t = np.ones(n, dtype)
    t[k] = v
    return t


BAD = {
    "n_fft = 32": (dict(n_fft=32, kind=np.ones(32, np.uint8), train=np.ones(32), pilot=None, cp=8), "n_fft = 32 must be a power of two"),
    "n_fft = 96": (dict(n_fft=96, kind=np.ones(96, np.uint8), train=np.ones(96), pilot=None), "n_fft = 96 must be a power of two"),
    "n_fft = 8192": (dict(n_fft=8192, kind=np.ones(8192, np.uint8), train=np.ones(8192), pilot=None), "n_fft = 8192 must be a power of two"),
    "cp = -1": (dict(cp=-1), "cp = -1 must be in [0, n_fft = 64]"),
    "cp = N + 1": (dict(cp=65), "cp = 65 must be in"),
    "advance = -1": (dict(advance=-1), "advance = -1 must be in [0, cp = 8]"),
    "advance = cp + 1": (dict(advance=9), "advance = 9 must be in"),
    "n_train = 0": (dict(n_train=0), "n_train = 0 must be in [1, 4]"),
    "n_train = 5": (dict(n_train=5), "n_train = 5 must be in"),
    "n_data = 0": (dict(n_data=0, pilot_sign=None), "n_data = 0 must be in [1, 4096]"),
    "n_data = 4097": (dict(n_data=4097, pilot_sign=None), "n_data = 4097 must be in"),
    "kind = 3": (dict(kind=_table(64, 9, 3, np.uint8)), "kind[9] = 3 must be 0"),
    "no data bin": (dict(kind=_table(64, slice(None), 2, np.uint8)), "kind names no data bin"),
    "train zero on a used bin": (dict(train=_table(64, 7, 0)), "train value 7 of a used bin is zero"),
    "train not finite": (dict(train=_table(64, 40, np.nan)), "train value 40 is not finite"),
    "pilot zero on a pilot bin": (dict(pilot=_table(64, 12, 0)), "pilot value 12 of a pilot bin is zero"),
    "pilot not finite": (dict(pilot=_table(64, 3, np.inf)), "pilot value 3 is not finite"),
    "pilot missing": (dict(pilot=None), "null pilot table with 2 pilot bins"),
    "pilot_sign = 0": (dict(pilot_sign=np.array([1, 0], np.int8)), "pilot_sign[1] = 0 must be +1 or -1"),
    "cfo_mode = 2": (dict(cfo_mode=2), "cfo_mode = 2 must be 0"),
    "cfo_mode 1 without a prefix": (dict(cp=0, advance=0, cfo_skip=0), "cfo_mode 1 needs cp >= 1"),
    "cfo_skip = cp": (dict(cfo_skip=8), "cfo_skip = 8 must be in [0, cp = 8)"),
    "cfo_skip = -1": (dict(cfo_skip=-1), "cfo_skip = -1 must be in"),
    "cfo_skip with cfo_mode 0": (dict(cfo_mode=0, cfo_skip=1), "cfo_skip = 1 must be in [0, cp = 8), and 0 with cfo_mode 0"),
    "out_mode = 2": (dict(out_mode=2), "out_mode = 2 must be SFE_OFDM_OUT_ZF"),
    "min_gate NaN": (dict(min_gate=np.nan), "min_gate must be finite"),
    "min_gate inf": (dict(min_gate=np.inf), "min_gate must be finite"),
}


@pytest.mark.parametrize("why", list(BAD))
def test_plan_and_create_refuse_a_bad_shape_with_its_message(api, lib, why):
    change, text = BAD[why]
    assert text in _refused(api, lib, **change)


def test_the_limits_themselves_are_taken_and_the_rest_of_the_refusals(api, lib):
    assert api.ofdm_plan(**_good()) is None
    assert api.ofdm_plan(**dict(_good(), cp=64, advance=64, n_train=4, n_data=4096, pilot_sign=None, cfo_skip=63, min_gate=-3.5)) is None
    assert api.ofdm_plan(**dict(_good(), cp=0, advance=0, cfo_mode=0, cfo_skip=0, out_mode=1)) is None
    big = np.ones(4096, np.uint8)
    assert api.ofdm_plan(4096, 4096, 0, 4, 4096, big, np.ones(4096, np.complex64)) is None        # no pilots: no pilot table
    # n_streams is create's alone; samples to receive need somewhere to put the symbols
    with pytest.raises(lib.SfeError) as e:
        api.Ofdm(n_streams=0, **_good())
    assert e.value.code == lib.SFE_EINVAL and "ofdm: n_streams = 0" in str(e.value)
    L, a = lib.load(), _good()
    head, keep, Nd = api._ofdm_shape(**a)
    x = np.zeros(2 * 400, F32)
    fp = C.POINTER(C.c_float)
    assert L.sfe_dsp_ofdm_plan(*head, x.ctypes.data_as(fp), 400, None, None, 1, 0, 0, None, None, None, None) == lib.SFE_EINVAL
    assert L.sfe_dsp_last_error().startswith(b"ofdm: null symbols")
    sym = np.zeros(2 * 2 * Nd, F32)
    for n_in, nb, base, step in ((1 << 31, 1, 0, 0), (400, 1 << 31, 0, 0), (400, 1, 2 ** 63 - 1, 0), (400, 2, 0, -2 ** 63)):
        assert L.sfe_dsp_ofdm_plan(*head, x.ctypes.data_as(fp), n_in, None, None, nb, base, step, sym.ctypes.data_as(fp), None, None,
                                   None) == lib.SFE_EINVAL
        assert L.sfe_dsp_last_error().startswith(b"ofdm: "), L.sfe_dsp_last_error()


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present: create succeeds there")
def test_create_without_gpu_is_enodev(api, lib):
    with pytest.raises(lib.SfeError) as e:
        api.Ofdm(**_good())
    assert e.value.code == lib.SFE_ENODEV


def _plan(api, name, out_mode=0, **kw):
    x, starts, sent = oc.stream(name)
    return api.ofdm_plan(x=x, idx=starts.astype(np.uint32), **oc.shape_args(name, out_mode), **kw)


@pytest.mark.parametrize("out_mode", [0, 1], ids=["zf", "mrc"])
@pytest.mark.parametrize("name", oc.NAMES)
def test_the_plan_agrees_with_the_numpy_reference(api, name, out_mode):
    """Symbols and chan to 1e-6 rel-RMS, the bar tests/test_burst_host.py sets between a plan and its numpy restatement;
    record words within 1e-6 + 1e-6 |want|."""
    sym, ch, rec, st = _plan(api, name, out_mode)
    wsym, wch, wrec, wst = oc.reference(name, out_mode)
    assert not st.any() and not wst.any()
    for b in range(len(st)):
        es, ec = oc.rel_rms(sym[b], wsym[b]), oc.rel_rms(ch[b], wch[b])
        d = np.abs(rec[b].astype(np.float64) - wrec[b])
        print("%s burst %d: symbols %.2e chan %.2e rel-RMS, record |diff| %s" % (name, b, es, ec, " ".join("%.1e" % v for v in d[:6])))
        assert es <= 1e-6 and ec <= 1e-6
        assert (d <= 1e-6 + 1e-6 * np.abs(wrec[b].astype(np.float64))).all(), d
        assert not _bits(rec[b, 6:]).any()
    kind = oc.tables(name)[0]
    assert not _bits(ch[:, kind == 0]).any()            # unused bins: +0


@pytest.mark.parametrize("out_mode", [0, 1], ids=["zf", "mrc"])
@pytest.mark.parametrize("name", oc.GRID_NAMES)
def test_the_plan_agrees_with_the_numpy_reference_over_the_grid(api, name, out_mode):
    """ofdm_cases.GRID -- every transform size with every bin used -- at the same bars: symbols (per burst and per data
    symbol's row) and chan to 1e-6 rel-RMS, record words within 1e-6 + 1e-6 |want|."""
    sym, ch, rec, st = _plan(api, name, out_mode)
    wsym, wch, wrec, wst = oc.reference(name, out_mode)
    assert not st.any() and not wst.any()
    for b in range(len(st)):
        rows = [oc.rel_rms(sym[b, j], wsym[b, j]) for j in range(sym.shape[1])]
        es, ec = oc.rel_rms(sym[b], wsym[b]), oc.rel_rms(ch[b], wch[b])
        d = np.abs(rec[b].astype(np.float64) - wrec[b])
        print("%s burst %d: symbols %.2e (worst row %.2e) chan %.2e rel-RMS, record |diff| %s" % (name, b, es, max(rows), ec, " ".join("%.1e" % v for v in d[:6])))
        assert es <= 1e-6 and ec <= 1e-6 and max(rows) <= 1e-6
        assert (d <= 1e-6 + 1e-6 * np.abs(wrec[b].astype(np.float64))).all(), d
        assert not _bits(rec[b, 6:]).any()
    assert not _bits(ch[:, oc.tables(name)[0] == 0]).any()


@pytest.mark.parametrize("name", oc.LONG_NAMES)
def test_the_plan_agrees_with_the_numpy_reference_on_the_long_burst(api, name):
    """1024 data symbols at eps = 0.4 and -0.47: the plan's eps within the record's bar of the reference's own, and then
    every row, chan and the record against the reference behind the plan's float32 eps (one ulp of eps moves arg phi_last
    by 3.8e-5 turns here, which is the hand-over's doing, not the law's), at the bars above."""
    x, starts, sent = oc.stream(name)
    for out_mode in (0, 1):
        sym, ch, rec, st = _plan(api, name, out_mode)
        own = oc.reference(name, out_mode)[2][0, 0]
        assert not st.any() and abs(float(rec[0, 0]) - float(own)) <= 1e-6 + 1e-6 * abs(float(own))
        wsym, wch, wrec, wst = synth.ofdm_reference(x, int(starts[0]), eps=rec[0, 0], **oc.reference_args(name, out_mode))
        assert wst == 0 and wrec[0] == rec[0, 0]
        rows = [oc.rel_rms(sym[0, j], wsym[j]) for j in range(wsym.shape[0])]
        d = np.abs(rec[0].astype(np.float64) - wrec)
        print("%s mode %d: eps %.9g (the reference's own %.9g), worst row %.2e, chan %.2e, record |diff| %s"
              % (name, out_mode, rec[0, 0], own, max(rows), oc.rel_rms(ch[0], wch), " ".join("%.1e" % v for v in d[:6])))
        assert max(rows) <= 1e-6 and oc.rel_rms(ch[0], wch) <= 1e-6
        assert (d <= 1e-6 + 1e-6 * np.abs(wrec.astype(np.float64))).all(), d
        assert np.array_equal(np.sign(sym[0].real), np.sign(sent[0].real)) and np.array_equal(np.sign(sym[0].imag), np.sign(sent[0].imag))


def test_the_reference_takes_a_handed_in_eps():
    """Without eps, and with its own estimate handed back in, the reference's bits are the same; another eps changes the
    rows and is the record's first word; with cfo_mode 0 it is not looked at."""
    name = "n64"
    x, starts, _ = oc.stream(name)
    a = oc.reference_args(name)
    own = synth.ofdm_reference(x, int(starts[0]), **a)
    again = synth.ofdm_reference(x, int(starts[0]), eps=own[2][0], **a)
    assert all(np.array_equal(_bits(u), _bits(v)) for u, v in zip(own[:3], again[:3])) and own[3] == again[3] == 0
    other = synth.ofdm_reference(x, int(starts[0]), eps=0.125, **a)
    assert other[2][0] == np.float32(0.125) and not np.array_equal(other[0], own[0])
    off = dict(a, cfo_mode=0, cfo_skip=0)
    assert all(np.array_equal(_bits(u), _bits(v)) for u, v in zip(synth.ofdm_reference(x, int(starts[0]), **off)[:3],
                                                                  synth.ofdm_reference(x, int(starts[0]), eps=0.3, **off)[:3]))


@pytest.mark.parametrize("name", ["g256", "g1024", "g2048"])
def test_the_exact_case_is_exact_in_the_plan_at_the_grid_sizes(api, name):
    test_the_exact_case_is_exact_in_the_plan(api, name)


@pytest.mark.parametrize("name", oc.NAMES)
def test_the_plan_recovers_the_sent_symbols_through_multipath(api, name):
    """Noiseless bursts through the shape's channel and offset: no symbol error in either output mode, the estimated
    offset is the applied one, and the worst error vector stays within twice what ofdm_cases.WORST records."""
    x, starts, sent = oc.stream(name)
    sym, ch, rec, st = _plan(api, name, 0)
    assert not st.any()
    worst = float(np.abs(sym - sent).max())
    print("%s: worst error vector %.3e (WORST %.3e), eps^ %s of %g, pilot error %s, min |H|^2 / h2 %s"
          % (name, worst, oc.WORST[name], rec[:, 0], oc.SHAPES[name]["eps"], rec[:, 3], rec[:, 2]))
    for got in (sym, _plan(api, name, 1)[0]):
        assert np.array_equal(np.sign(got.real), np.sign(sent.real)) and np.array_equal(np.sign(got.imag), np.sign(sent.imag))
    assert worst <= 2 * oc.WORST[name]
    assert np.abs(rec[:, 0] - oc.SHAPES[name]["eps"]).max() <= 1e-4
    # H is the channel's response, turned by the window's advance
    N, g = oc.SHAPES[name]["n_fft"], oc.SHAPES[name]["advance"]
    used = oc.tables(name)[0] != 0
    resp = np.fft.fft(oc.channel(name), N) * np.exp(-2j * np.pi * np.arange(N) * g / N)
    assert oc.rel_rms(ch[0, used], resp[used]) <= max(2 * oc.WORST[name], 1e-4)


@pytest.mark.parametrize("name", oc.NAMES)
def test_the_exact_case_is_exact_in_the_plan(api, name):
    a, x, starts = oc.exact_case(name)
    used = a["kind"] != 0
    for out_mode in (0, 1):
        sym, ch, rec, st = api.ofdm_plan(x=x, idx=starts.astype(np.uint32), out_mode=out_mode, **a)
        assert not st.any()
        assert np.array_equal(_bits(sym), _bits(np.ones_like(sym)))
        assert np.array_equal(_bits(ch[:, used]), _bits(np.ones_like(ch[:, used]))) and not _bits(ch[:, ~used]).any()
        assert np.array_equal(_bits(rec), _bits(np.tile(np.array([0, 1, 1, 0, 0, 0, 0, 0], F32), (len(st), 1))))


def _failed(sym, ch, rec, b):
    return (not _bits(sym[b]).any() and not _bits(ch[b]).any() and np.isnan(rec[b, :6]).all()
            and ((_bits(rec[b, :6]) & 0x7fc00000) == 0x7fc00000).all() and not _bits(rec[b, 6:]).any())


def test_statuses_1_2_and_3_each_from_its_own_cause(api):
    name = "n64"
    x, starts, sent = oc.stream(name)
    a = oc.shape_args(name, 0, min_gate=0.5)
    R, N, cp = oc.reach(name), 64, 16
    clean = api.ofdm_plan(x=x, idx=starts.astype(np.uint32), **a)
    assert not clean[3].any()

    def one(xx, o, gate=None, **kw):
        return api.ofdm_plan(x=xx, start_base=int(o), gate=None if gate is None else [gate], **dict(a, **kw))

    o = int(starts[1])
    # status 2: the gate, a NaN gate; a gate at the bar passes
    for g, want in ((0.25, 2), (np.nan, 2), (0.5, 0)):
        r = one(x, o, g)
        assert r[3].tolist() == [want] and (_failed(*r[:3], 0) if want else np.array_equal(_bits(r[0][0]), _bits(clean[0][1])))
    # status 3: the range's two edges, one sample each way
    seg = np.array(x[o:o + R])
    assert one(seg, 0)[3].tolist() == [0] and one(seg, -1)[3].tolist() == [3] and one(seg, 1)[3].tolist() == [3]
    assert one(np.array(x[o:o + R + 1]), 1)[3].tolist() == [0]
    assert _failed(*one(seg, 1)[:3], 0) and one(seg, -2 ** 40)[3].tolist() == [3] and one(seg, 2 ** 40)[3].tolist() == [3]
    # a gated burst out of range is gated: neither reads a sample
    assert one(seg, 1, 0.0)[3].tolist() == [2]
    # status 1: a non-finite sample at either end of the reach, outside every window (the first cp - g samples of a symbol
    # are in none); one sample beyond the reach is not the burst's
    for at, val, want in ((o, complex(np.nan, 0), 1), (o + R - 1, complex(0, np.inf), 1), (o + 2, complex(0, -np.inf), 1), (o - 1, np.nan, 0),
                          (o + R, np.nan, 0)):
        bad = np.array(x)
        bad[at] = val
        r = one(bad, o)
        assert r[3].tolist() == [want], (at, val)
        assert _failed(*r[:3], 0) if want else np.array_equal(_bits(r[0][0]), _bits(clean[0][1]))
    # status 1: gamma = 0 (silence in every prefix with cfo_mode 1) ...
    silent = np.array(seg)
    for j in range(8):
        silent[j * (N + cp):j * (N + cp) + cp] = 0
    assert one(silent, 0)[3].tolist() == [1] and one(silent, 0, cfo_mode=0, cfo_skip=0)[3].tolist() == [0]
    # ... a used bin with H = 0 (training symbols of silence) ...
    mute = np.array(seg)
    mute[:2 * (N + cp)] = 0
    r = one(mute, 0, cfo_mode=0, cfo_skip=0)
    assert r[3].tolist() == [1] and _failed(*r[:3], 0)
    # ... and P_j = 0: the last data symbol silent (its rows before it were computed and are taken back)
    last = np.array(seg)
    last[7 * (N + cp):] = 0
    r = one(last, 0, cfo_mode=0, cfo_skip=0)
    assert r[3].tolist() == [1] and _failed(*r[:3], 0)
    # neighbours of a failed burst are untouched
    bad = np.array(x)
    bad[o + 5] = np.nan
    r = api.ofdm_plan(x=bad, idx=starts.astype(np.uint32), gate=[1, 1, 0.1], **a)
    assert r[3].tolist() == [0, 1, 2] and _failed(*r[:3], 1) and _failed(*r[:3], 2)
    for u, v in zip(r[:3], clean[:3]):
        assert np.array_equal(_bits(u[0]), _bits(v[0]))


def test_signal_maps_bits_as_the_modulator_does():
    """synth.ofdm_signal takes bits or symbols: the bits go through synth.mod_symbols' Gray QPSK."""
    name = "n64"
    sh = oc.SHAPES[name]
    kind, train, pilot, sign = oc.tables(name)
    Nd = oc.n_data_bins(name)
    bits = synth.vit_bits(2 * sh["n_data"] * Nd, seed=5)
    kw = dict(pilot=pilot, pilot_sign=sign, taps=oc.channel(name), eps=0.05)
    a = synth.ofdm_signal(64, 16, 2, kind, train, 900, 7, bits=bits, **kw)
    b = synth.ofdm_signal(64, 16, 2, kind, train, 900, 7, symbols=synth.mod_symbols(bits, 4, 1.0).reshape(-1, Nd), **kw)
    assert a.dtype == np.complex64 and np.array_equal(a, b) and not a[:7].any() and a[7:7 + oc.reach(name)].all()
