"""The burst demodulator (sfe_dsp_burst_*) without a GPU: the C ABI's declarations and exports, the host-only planner --
its refusals, its float64 law against an independent numpy restatement written here, what it recovers from pulse-shaped
PSK bursts of known timing and carrier, the `given` path, the exact constant case, the gate, the range and its two edges,
a NaN sample -- the no-GPU refusal and the build lists."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from simplefe_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "sfe_dsp.h")
BURST_FUNCS = ("sfe_dsp_burst_plan", "sfe_dsp_burst_create", "sfe_dsp_burst_set_input_format", "sfe_dsp_burst_set_gate",
               "sfe_dsp_burst_process_stream", "sfe_dsp_burst_destroy")
FP = C.POINTER(C.c_float)
F32 = np.float32
# (sps, N, Lp, lag)
SHAPES = [(4, 32, 8, 1), (10, 256, 32, 4), (50, 64, 16, 2), (64, 16, 4, 1), (4, 4096, 64, 8)]
SHAPE_IDS = ["sps%d-N%d-Lp%d-lag%d" % s for s in SHAPES]
# The plan's worst errors over a shape's cases, measured here on the CPU (DESIGN.md 4.16 quotes them): the cut pulses'
# pull on the timing estimate, what that and the preamble's length leave of the carrier estimate, and the cubic
# interpolator's error -- all properties of the law.  The tests assert twice these.
#        |tau^ - tau| samples, |f^ - f| turns per symbol, EVM: rel-RMS over a burst's N symbols
WORST = {(4, 32, 8, 1): (7.58e-2, 2.91e-4, 3.45e-2), (10, 256, 32, 4): (4.59e-2, 2.16e-6, 6.24e-3), (50, 64, 16, 2): (1.46, 5.94e-5, 3.81e-2),
         (64, 16, 4, 1): (3.21, 3.53e-3, 2.15e-1), (4, 4096, 64, 8): (9.23e-4, 1.14e-6, 1.69e-2)}

# The payload of a shape (one BPSK and one QPSK sequence, shared by its cases) is drawn from SEED + PAYLOAD[shape].  An
# isolated burst's first pulse is cut by the start of the timing window when tau < 0, which moves tau^ by up to 0.06 sps at
# N = 16 and N = 32 and 0.02 sps at N = 64 -- towards 0 or away from it, as the first symbols have it.  At tau = -0.49 sps, 0.01 sps
# away from the cut of the estimator's range, "away" means tau^ = tau + sps: the burst is taken one symbol late, which is
# what the law says of such a burst and not a recovery.  About half of all payloads do that at the three short shapes; these
# do not (the first offset per shape at which neither sequence does), so that every case of the list is a recovery.
PAYLOAD = [0, 1, 5, 6, 4]


@pytest.fixture(scope="module")
def L():
    from simplefe_amd import lib
    return lib.load()


_cases = {}


def cases(shape):
    """synth.burst_cases of a shape: per (tau, f), (x complex64, o, the transmitted symbols, tau, f, phase, amp)."""
    if shape not in _cases:
        sps, N, Lp, lag = shape
        _cases[shape] = synth.burst_cases(sps, N, lag, seed=synth.SEED + PAYLOAD[SHAPES.index(shape)])
    return _cases[shape]


def law64(x, o, pre, sps, N, lag, timing_mode=0):
    """The law of include/sfe_dsp.h on one burst in numpy float64, independent of the library: (symbols complex128,
    record float64[8]).  The estimates are rounded to float32 where the law hands them on."""
    x = np.asarray(x, np.complex128)
    pre = np.asarray(pre, np.complex128)
    Lp, E_p = pre.size, float(F32((np.abs(pre) ** 2).sum()))
    tau = F32(0.0)
    if timing_mode == 0:
        i = np.arange(N * sps)
        c = (np.abs(x[o + i]) ** 2 * np.exp(-2j * np.pi * (i % sps) / sps)).sum()
        t = -sps * np.angle(c) / (2 * np.pi)
        tau = F32(t + sps if t <= -0.5 * sps else t)
    m = int(np.floor(float(tau)))
    mu = float(tau) - m
    lag4 = [-mu * (mu - 1) * (mu - 2) / 6, (mu + 1) * (mu - 1) * (mu - 2) / 2, -(mu + 1) * mu * (mu - 2) / 2, (mu + 1) * mu * (mu - 1) / 6]
    at = o + np.arange(N) * sps + m
    y = sum(lag4[q + 1] * x[at + q] for q in (-1, 0, 1, 2))
    z = y[:Lp] * np.conj(pre)
    R = (z[lag:] * np.conj(z[:-lag])).sum()
    f = F32(np.angle(R) / (2 * np.pi * lag))

    def unturn(t):
        return np.exp(-2j * np.pi * (t - np.rint(t)))

    k = np.arange(N, dtype=np.float64)
    S = (z * unturn(float(f) * k[:Lp])).sum()
    theta, a = F32(np.angle(S) / (2 * np.pi)), F32(abs(S) / E_p)
    sym = y * unturn(float(theta) + float(f) * k) / float(a)
    rec = np.array([tau, f, theta, a, abs(S) ** 2 / (E_p * (np.abs(y[:Lp]) ** 2).sum()), (np.abs(sym[:Lp] - pre) ** 2).sum() / E_p, 0, 0])
    return sym, rec


def _pre(n):
    p = np.zeros((n, 2), F32)
    p[:, 0] = 1.0
    return p


def _plan_rc(L, pre, sps, N, lag, mode=0, gate=0.0):
    return L.sfe_dsp_burst_plan(pre.ctypes.data_as(FP) if pre is not None else None, 0 if pre is None else len(pre), sps, N, lag, mode, gate,
                                None, 0, None, None, 0, 0, 0, None, None, None, None)


def _create_rc(L, pre, sps, N, lag, mode=0, gate=0.0, n_streams=1):
    h = C.c_void_p()
    rc = L.sfe_dsp_burst_create(pre.ctypes.data_as(FP) if pre is not None else None, 0 if pre is None else len(pre), sps, N, lag, mode, gate,
                                n_streams, 0, C.byref(h))
    return rc, h.value


def _refused(L, pre, sps, N, lag, **kw):
    """Plan and create both refuse with a "burst: " message; create does so before it looks for a device."""
    from simplefe_amd import lib
    assert _plan_rc(L, pre, sps, N, lag, **kw) == lib.SFE_EINVAL
    assert L.sfe_dsp_last_error().startswith(b"burst: "), L.sfe_dsp_last_error()
    rc, h = _create_rc(L, pre, sps, N, lag, **kw)
    assert rc == lib.SFE_EINVAL and not h
    assert L.sfe_dsp_last_error().startswith(b"burst: "), L.sfe_dsp_last_error()


def test_header_declares_burst_abi_and_library_exports_it(L):
    from simplefe_amd import lib
    declared = set(re.findall(r"\b(sfe_dsp_burst_[a-z0-9_]+)\s*\(", open(HDR).read()))
    assert declared == set(BURST_FUNCS)
    for name in BURST_FUNCS:
        assert hasattr(L, name), name
        assert name in lib.SIGNATURES, name


BAD = {"sps = 3": (8, 3, 16, 1), "sps = 65": (8, 65, 16, 1), "N = 1": (2, 8, 1, 1), "N = 4097": (8, 8, 4097, 1), "Lp = 1": (1, 8, 16, 1),
       "Lp = N + 1": (17, 8, 16, 1), "lag = 0": (8, 8, 16, 0), "lag = Lp": (8, 8, 16, 8)}


@pytest.mark.parametrize("why", list(BAD))
def test_plan_and_create_refuse_a_bad_shape_with_a_message(L, why):
    Lp, sps, N, lag = BAD[why]
    _refused(L, _pre(Lp), sps, N, lag)


def test_plan_and_create_refuse_bad_values(L):
    from simplefe_amd import lib
    good = _pre(8)
    assert _plan_rc(L, good, 8, 16, 1) == lib.SFE_OK
    assert _plan_rc(L, good, 4, 8, 7, 1, -3.5) == lib.SFE_OK      # the limits themselves: sps 4, Lp = N, lag = Lp - 1
    assert _plan_rc(L, _pre(2), 64, 4096, 1) == lib.SFE_OK
    for bad in (np.nan, np.inf, -np.inf):
        p = good.copy()
        p[5, 1] = bad
        _refused(L, p, 8, 16, 1)
        _refused(L, good, 8, 16, 1, gate=bad)
    _refused(L, np.zeros((8, 2), F32), 8, 16, 1)                  # an all-zero preamble: E_p = 0
    _refused(L, None, 8, 16, 1)
    _refused(L, good, 8, 16, 1, mode=2)
    _refused(L, good, 8, 16, 1, mode=-1)
    rc, h = _create_rc(L, good, 8, 16, 1, n_streams=0)
    assert rc == lib.SFE_EINVAL and not h and L.sfe_dsp_last_error().startswith(b"burst: ")
    # samples to demodulate need somewhere to put the symbols
    x = np.ones(2 * 18 * 8, F32)
    assert L.sfe_dsp_burst_plan(good.ctypes.data_as(FP), 8, 8, 16, 1, 0, 0.0, x.ctypes.data_as(FP), 18 * 8, None, None, 1, 8, 0, None, None,
                                None, None) == lib.SFE_EINVAL
    assert L.sfe_dsp_last_error().startswith(b"burst: ")


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present: create succeeds there")
def test_create_without_gpu_is_enodev():
    from simplefe_amd import api, lib
    with pytest.raises(lib.SfeError) as e:
        api.Burst(np.ones(8, np.complex64), 8, 16, 1)
    assert e.value.code == lib.SFE_ENODEV


def _rel_rms(got, want):
    return float(np.sqrt((np.abs(np.asarray(got, np.complex128) - want) ** 2).sum() / (np.abs(want) ** 2).sum()))


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_plan_agrees_with_the_numpy_restatement(shape):
    from simplefe_amd import api
    sps, N, Lp, lag = shape
    for x, o, a, tau, f, phase, amp in cases(shape):
        sym, rec, st = api.burst_plan(a[:Lp], sps, N, lag, x=x, start_base=o)
        want_sym, want_rec = law64(x, o, a[:Lp].astype(np.complex64), sps, N, lag)
        assert st[0] == 0
        err = np.abs(rec[0].astype(np.float64) - want_rec)
        print("tau %+.3f f %+.3f: record |diff| max %.2e, symbols rel-RMS %.2e" % (tau, f, err.max(), _rel_rms(sym[0], want_sym)))
        assert err.max() <= 1e-6, (tau, f, rec[0], want_rec)
        assert _rel_rms(sym[0], want_sym) <= 1e-6, (tau, f)
        assert rec[0, 6:].view(np.uint32).tolist() == [0, 0]


def measure_recovery(shape):
    """Worst |tau^ - tau|, |f^ - f| and symbol EVM (rel-RMS over the N symbols) of the plan over a shape's cases."""
    from simplefe_amd import api
    sps, N, Lp, lag = shape
    worst = np.zeros(3)
    for x, o, a, tau, f, phase, amp in cases(shape):
        sym, rec, st = api.burst_plan(a[:Lp], sps, N, lag, x=x, start_base=o)
        assert st[0] == 0
        worst = np.maximum(worst, [abs(rec[0, 0] - tau), abs(rec[0, 1] - f), _rel_rms(sym[0], a)])
    return worst


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_plan_recovers_the_transmitted_symbols(shape):
    from simplefe_amd import api
    sps, N, Lp, lag = shape
    worst = measure_recovery(shape)
    print("worst |tau^ - tau| %.3e samples, |f^ - f| %.3e turns/symbol, EVM %.3e" % tuple(worst))
    assert (worst <= 2 * np.array(WORST[shape])).all(), worst
    # the decisions are the transmitted symbols, both components of every symbol of every case (BPSK: the real one, its
    # imaginary part is zero); phase and amplitude come back too
    for x, o, a, tau, f, phase, amp in cases(shape):
        sym, rec, st = api.burst_plan(a[:Lp], sps, N, lag, x=x, start_base=o)
        want = a.round(6)
        assert np.array_equal(np.sign(sym[0].real), np.sign(want.real)), (tau, f)
        if want.imag.any():
            assert np.array_equal(np.sign(sym[0].imag), np.sign(want.imag)), (tau, f)
        # theta is the phase at symbol 0 of a fit over Lp symbols: off by at most the frequency error grown over the
        # preamble plus what the symbol error (the EVM, in radians) leaves; the amplitude by the EVM
        dphi = np.angle(np.exp(1j * (2 * np.pi * rec[0, 2] - phase)))
        assert abs(dphi) <= 2 * np.pi * (2 * WORST[shape][1]) * Lp + 2 * WORST[shape][2] and abs(rec[0, 3] / amp - 1) <= 2 * WORST[shape][2]


# (shape, seed offset, order) of payloads that do slip: found beside PAYLOAD, the BPSK sequences of the offsets before it
SLIPS = [((50, 64, 16, 2), 2, 2), ((64, 16, 4, 1), 3, 2), ((4, 32, 8, 1), 2, 2)]


@pytest.mark.parametrize("shape,offset,order", SLIPS, ids=["sps%d-N%d" % s[0][:2] for s in SLIPS])
def test_a_burst_at_the_cut_of_the_timing_range_may_come_out_one_symbol_late(shape, offset, order):
    """What PAYLOAD avoids, pinned: at tau = -0.49 sps these payloads' cut first pulse pushes the estimate across -sps/2, and
    the law answers tau + sps -- the same sampling instants, counted from one symbol later: y[k] is symbol k + 1.  At
    tau = +0.49 sps, where no pulse is cut, the same payloads are recovered."""
    from simplefe_amd import api
    sps, N, Lp, lag = shape
    a = synth.psk_symbols(N, order, seed=synth.SEED + offset)
    o, n, tau = 3 * sps + 5, (N + 8) * sps + 11, -0.49 * sps
    x = synth.burst_signal(a, sps, n, o, tau, 0.0, 0.4, 1.0)
    rec = api.burst_plan(a[:Lp], sps, N, lag, x=x, start_base=o)[1]
    print("tau %.3f, tau^ %.3f = tau + sps %+.3f" % (tau, rec[0, 0], rec[0, 0] - tau - sps))
    # a statement of side, not of accuracy: the estimate lies beyond the cut, nearer to +sps/2 than to 0, where tau + sps is
    assert 0.25 * sps < rec[0, 0] <= 0.5 * sps and rec[0, 0] < tau + sps
    # told that the burst is the one a symbol later, the same samples are that burst at tau^ - sps ... which is tau
    late = api.burst_plan(a[1:Lp + 1], sps, N - 1, lag, x=x, start_base=o)
    assert late[2][0] == 0 and 0.25 * sps < late[1][0, 0] <= 0.5 * sps
    assert np.array_equal(np.sign(late[0][0].real), np.sign(a[1:].real.round(6)))
    rec = api.burst_plan(a[:Lp], sps, N, lag, x=synth.burst_signal(a, sps, n, o, -tau, 0.0, 0.4, 1.0), start_base=o)[1]
    assert abs(rec[0, 0] + tau) <= 2 * WORST[shape][0]


def test_given_estimates_reproduce_the_plans_own_symbols():
    from simplefe_amd import api
    sps, N, Lp, lag = SHAPES[1]
    x, o, a = cases(SHAPES[1])[6][:3]
    sym, rec, st = api.burst_plan(a[:Lp], sps, N, lag, x=x, start_base=o)
    sym2, rec2, st2 = api.burst_plan(a[:Lp], sps, N, lag, x=x, start_base=o, given=rec)
    assert st2[0] == 0 and np.array_equal(sym.view(np.uint32), sym2.view(np.uint32))
    assert np.array_equal(rec[:, :4].view(np.uint32), rec2[:, :4].view(np.uint32)) and np.allclose(rec[:, 4:], rec2[:, 4:], rtol=1e-6, atol=1e-9)
    # other estimates give other symbols: a quarter turn more of phase turns every symbol back by a quarter turn
    turned = rec.copy()
    turned[0, 2] += 0.25
    sym3 = api.burst_plan(a[:Lp], sps, N, lag, x=x, start_base=o, given=turned)[0]
    assert _rel_rms(sym3[0], -1j * sym[0].astype(np.complex128)) <= 1e-6
    bad = rec.copy()
    bad[0, 3] = np.nan
    sym4, rec4, st4 = api.burst_plan(a[:Lp], sps, N, lag, x=x, start_base=o, given=bad)
    assert st4[0] == 1 and not sym4.view(np.uint32).any() and np.isnan(rec4[0, :6]).all()


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_the_constant_case_is_exact(shape):
    """Contract 4: timing_mode 1, p all ones, x = 1+0j: f = theta = +0, a = q = 1, evm = 0, y^ exactly 1+0j."""
    from simplefe_amd import api
    sps, N, Lp, lag = shape
    x = np.ones((N + 2) * sps, np.complex64)
    sym, rec, st = api.burst_plan(np.ones(Lp), sps, N, lag, timing_mode=1, x=x, start_base=sps)
    assert st[0] == 0 and np.array_equal(sym[0], np.ones(N, np.complex64))
    assert rec[0].view(np.uint32).tolist() == np.array([0, 0, 0, 1, 1, 0, 0, 0], F32).view(np.uint32).tolist()


def test_gate_range_and_nan_statuses():
    from simplefe_amd import api
    sps, N, Lp, lag = SHAPES[0]
    x, o, a = cases(SHAPES[0])[9][:3]
    reach_end = o + (N + 1) * sps
    pre = a[:Lp]
    good = api.burst_plan(pre, sps, N, lag, x=x, start_base=o)
    # five bursts at the same place through the index table: good, gated, NaN gate, before the buffer, good
    idx = np.array([o, o, o, sps - 1, o], np.uint32)
    gate = np.array([0.5, 0.25, np.nan, 0.9, 0.9], F32)
    sym, rec, st = api.burst_plan(pre, sps, N, lag, min_gate=0.5, x=x, idx=idx, gate=gate)
    assert st.tolist() == [0, 2, 2, 3, 0]
    for b in (0, 4):
        assert np.array_equal(sym[b].view(np.uint32), good[0][0].view(np.uint32)) and np.array_equal(rec[b].view(np.uint32), good[1][0].view(np.uint32))
    for b in (1, 2, 3):
        assert not sym[b].view(np.uint32).any() and np.isnan(rec[b, :6]).all() and rec[b, 6:].view(np.uint32).tolist() == [0, 0]
    # a gated burst is not looked at: out of range and gated is gated
    assert api.burst_plan(pre, sps, N, lag, min_gate=0.5, x=x, idx=[0], gate=[0.0])[2][0] == 2
    # the reach may end exactly at n_in and begin exactly at 0; one sample beyond either is status 3
    assert api.burst_plan(pre, sps, N, lag, x=x[:reach_end], start_base=o)[2][0] == 0
    assert api.burst_plan(pre, sps, N, lag, x=x[:reach_end - 1], start_base=o)[2][0] == 3
    assert api.burst_plan(pre, sps, N, lag, x=x[o - sps:], start_base=sps)[2][0] == 0
    assert api.burst_plan(pre, sps, N, lag, x=x[o - sps + 1:], start_base=sps - 1)[2][0] == 3
    assert api.burst_plan(pre, sps, N, lag, x=x, start_base=-5)[2][0] == 3
    # start_base, start_step and idx add up in signed 64-bit arithmetic
    far = api.burst_plan(pre, sps, N, lag, x=x, idx=[o + 7, o + 7], start_base=-7 - 3 * 10 ** 12, start_step=3 * 10 ** 12, n_bursts=2)
    assert far[2].tolist() == [3, 0] and np.array_equal(far[0][1].view(np.uint32), good[0][0].view(np.uint32))
    two = api.burst_plan(pre, sps, N, lag, x=x, idx=[o + 7, o + 4], start_base=-7, start_step=3, n_bursts=2)
    assert two[2].tolist() == [0, 0] and np.array_equal(two[0][1].view(np.uint32), good[0][0].view(np.uint32))
    # ... and what cannot be added up in signed 64-bit arithmetic is refused
    from simplefe_amd import lib
    for base, step, nb in ((2 ** 63 - 1, 0, 1), (-2 ** 63, 0, 1), (0, 2 ** 62, 3), (0, -2 ** 62, 3), (2 ** 63 - 2 ** 33 + 1, 0, 1)):
        with pytest.raises(lib.SfeError) as e:
            api.burst_plan(pre, sps, N, lag, x=x, start_base=base, start_step=step, n_bursts=nb)
        assert e.value.code == lib.SFE_EINVAL and "burst: " in str(e.value)
    assert api.burst_plan(pre, sps, N, lag, x=x, start_base=2 ** 63 - 2 ** 33, start_step=-2 ** 61, n_bursts=2)[2].tolist() == [3, 3]
    # a non-finite sample anywhere in the reach, its first and last samples included, fails the burst; one outside does not
    for at, want in ((o - sps, 1), (o + 17, 1), (reach_end - 1, 1), (o - sps - 1, 0), (reach_end, 0)):
        for bad in (np.nan, np.inf):
            xb = x.copy()
            xb[at] = complex(0.0, bad)
            for mode in (0, 1):
                s2, r2, t2 = api.burst_plan(pre, sps, N, lag, timing_mode=mode, x=xb, start_base=o)
                assert t2[0] == want, (at, bad, mode)
                if want:
                    assert not s2.view(np.uint32).any() and np.isnan(r2[0, :6]).all()


def test_build_lists_name_the_burst_files():
    from simplefe_amd import build
    assert "api_burst.hip" in build.HOST_SOURCES and "burst.hip" in build.EXACT_SOURCES and build.SCRATCH_FREE["burst.hip"]
    assert build.KERNEL_FILES["burst"][:2] == ("burst.hip", "burst.h")
    assert "burst.hip" in open(os.path.join(ROOT, "CMakeLists.txt")).read()
