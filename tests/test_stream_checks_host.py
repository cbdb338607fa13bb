"""Negative controls for tests/stream_checks.py, on the CPU: the oracle's own output plays the device result, laid into
poisoned, guarded buffers the way the GPU runners lay them; the verdict functions pass it, and every corruption a
subtly wrong kernel or host law could produce makes the NAMED check raise.  And the other direction: the per-sample
bounds are not so tight that a correct float32 implementation fails them (the float32 oracle against a float64
direct sum; float32 overlap-save by scipy.fft against a float64 convolution)."""
import types

import numpy as np
import pytest

import stream_checks as sc
from simplefe_amd import synth

B = 4096
TAPS, U = synth.taps_cfg3(), 3                      # 381 taps, 127 per phase
NCH = 2


class Stream:
    """Two channels of one stream through the oracle, call by call, and their images in guarded buffers."""

    def __init__(self, orc, rate, n, cuts):
        self.rate, self.n, self.cuts = float(np.float32(rate)), n, cuts
        self.S = sc.int_step(self.rate, U)
        self.x = np.stack([synth.synth_f32(n, ch=40 + c) for c in range(NCH)])
        per = [sc.reference_stream(orc.Resample(TAPS, U, B), self.x[c], self.rate, cuts, B) for c in range(NCH)]
        self.ref = np.stack([p[0] for p in per])
        self.ref_counts = per[0][1]
        assert per[1][1] == self.ref_counts
        o = orc.Resample(TAPS, U, B)
        sc.reference_stream(o, self.x[0], self.rate, cuts, B)
        self.state = types.SimpleNamespace(leftover=o.get_time()[2])
        self.A = np.stack([sc.reference_stream(orc.Resample(np.abs(TAPS), U, B), np.abs(self.x[c]), self.rate, cuts, B)[0]
                           for c in range(NCH)])
        self.bound = sc.direct_bound(self.A, 127)

    def device(self, x=None, orc=None):
        """What the runner would read back after each call: [(out_raw, out_layout, k, in_after, in_before)]."""
        ref = self.ref if x is None else np.stack([sc.reference_stream(orc.Resample(TAPS, U, B), x[c], self.rate, self.cuts, B)[0]
                                                   for c in range(NCH)])
        calls, k0 = [], 0
        for (a, b), k in zip(zip(self.cuts[:-1], self.cuts[1:]), self.ref_counts):
            ilay, iraw = sc._lay_input(self.x, NCH, 4, a, b, True)
            olay = sc.out_layout(NCH, 4, int(np.ceil((b - a) / self.rate)) + 4)
            oraw = olay.poisoned()
            for c in range(NCH):
                olay.put(oraw, c, ref[c, k0:k0 + k])
            calls.append([oraw, olay, k, iraw.copy(), iraw])
            k0 += k
        return calls

    def judge(self, calls, exact, state=None, counts_only_total=False):
        """Everything a routed GPU test applies; returns the worst per-sample ratio."""
        got = []
        for oraw, olay, k, iafter, ibefore in calls:
            sc.check_written(oraw, olay, k)
            sc.check_input_intact(iafter, ibefore)
            got.append(np.stack([olay.take(oraw, c, k) for c in range(NCH)]))
        counts = [c[2] for c in calls]
        sc.check_counts(counts, sum(self.ref_counts) if counts_only_total else self.ref_counts,
                        self.state if state is None else state, self.n, U, self.S)
        got = np.concatenate(got, axis=1)
        return sc.check_values(got, self.ref, exact=exact, bound=None if exact else self.bound)


CUTS = [0, 1, B, 8000]


@pytest.fixture(scope="module")
def streams(orc):
    return {"integer": Stream(orc, 5.0 / 3.0, 8000, CUTS), "general": Stream(orc, 1.77, 8000, CUTS)}


KINDS = ["integer", "general"]


@pytest.mark.parametrize("kind", KINDS)
def test_the_verdicts_pass_the_oracles_own_output(streams, kind):
    s = streams[kind]
    assert len(s.ref_counts) == 3 and s.ref_counts[-1] > 100
    assert s.judge(s.device(), exact=True) == 0.0
    assert s.judge(s.device(), exact=False) == 0.0


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("exact", [True, False])
def test_output_shifted_by_one_sample(streams, kind, exact):
    s = streams[kind]
    calls = s.device()
    oraw, olay, k = calls[2][:3]
    for c in range(NCH):
        y = olay.take(oraw, c, k)
        olay.put(oraw, c, np.concatenate([y[:1], y[:-1]]))
    with pytest.raises(sc.ValuesError):
        s.judge(calls, exact=exact)


@pytest.mark.parametrize("kind", KINDS)
def test_last_output_of_each_call_left_as_poison(streams, kind):
    s = streams[kind]
    calls = s.device()
    for oraw, olay, k in (c[:3] for c in calls):
        if k:
            olay.put(oraw, NCH - 1, np.array([sc.POISON], np.uint32), at_item=k - 1)
    with pytest.raises(sc.WrittenError, match="never stored"):
        s.judge(calls, exact=True)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("exact", [True, False])
def test_last_output_of_each_call_is_the_previous_calls_last_value(streams, kind, exact):
    """What an unpoisoned, reused buffer lets through: the store was skipped and an old, plausible value is read back."""
    s = streams[kind]
    calls = s.device()
    prev = None
    for oraw, olay, k in (c[:3] for c in calls):
        if k == 0:
            continue
        last = [olay.take(oraw, c, k)[-1:].copy() for c in range(NCH)]
        if prev is not None:
            for c in range(NCH):
                olay.put(oraw, c, prev[c], at_item=k - 1)
        prev = last
    with pytest.raises(sc.ValuesError) as e:
        s.judge(calls, exact=exact)
    assert e.value.gate in (("exact",) if exact else ("rms", "sample"))


@pytest.mark.parametrize("n, pending", [(8000, False), (8002, True)])
@pytest.mark.parametrize("per_call", [True, False])
def test_reported_count_one_short_with_right_values(orc, n, pending, per_call):
    """The law that drops a stream's last output -- what `len(ref) - len(got) in (0, 1)` let pass -- with the stream
    ending on a pending leftover and without one."""
    s = Stream(orc, 5.0 / 3.0, n, [0, 1, B, n])
    assert bool(s.state.leftover) == pending
    K = sc.closed_form_total(n, U, 5)
    assert sum(s.ref_counts) == K and (K * 5 - n * U == -1) == pending
    s.judge(s.device(), exact=True, counts_only_total=not per_call)
    calls = s.device()
    oraw, olay, k = calls[2][:3]
    for c in range(NCH):
        olay.put(oraw, c, np.array([sc.POISON], np.uint32), at_item=k - 1)        # not stored, and not reported either
    calls[2][2] = k - 1
    for leftover in (0, 1):                      # whatever such a law says about its own state
        with pytest.raises(sc.CountError):
            s.judge(calls, exact=True, state=types.SimpleNamespace(leftover=leftover), counts_only_total=not per_call)


def test_a_leftover_flag_that_contradicts_the_count(streams):
    s = streams["integer"]
    with pytest.raises(sc.CountError, match="leftover"):
        s.judge(s.device(), exact=True, state=types.SimpleNamespace(leftover=1 - s.state.leftover))


def test_general_rate_count_one_short(streams):
    s = streams["general"]
    calls = s.device()
    calls[1][2] -= 1
    with pytest.raises(sc.CountError):
        s.judge(calls, exact=True)


def _stray(streams, kind, where):
    s = streams[kind]
    calls = s.device()
    oraw, olay = calls[2][:2]
    b = oraw.view(np.uint8)
    byte = {"at out_cap": olay.start(NCH - 1) + olay.cap,
            "front guard": olay.front - 4,
            "first word of the buffer": 0,
            "gap": olay.start(0) + olay.cap,
            "last word of the gap": olay.start(1) - 4,
            "last word of the buffer": olay.total - 4}[where]
    b[byte:byte + 4] = np.array([1.0], np.float32).view(np.uint8)
    return s, calls


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("where, named", [("at out_cap", "tail guard"), ("last word of the buffer", "tail guard"),
                                          ("front guard", "front guard"), ("first word of the buffer", "front guard"),
                                          ("gap", "gap after channel 0"), ("last word of the gap", "gap after channel 0")])
def test_one_word_written_outside_the_declared_range(streams, kind, where, named):
    s, calls = _stray(streams, kind, where)
    with pytest.raises(sc.WrittenError, match=named):
        s.judge(calls, exact=True)


@pytest.mark.parametrize("kind", KINDS)
def test_words_between_the_count_and_out_cap_are_free(streams, kind):
    """include/sfe_dsp.h: up to out_cap outputs per channel may be written."""
    s = streams[kind]
    calls = s.device()
    oraw, olay, k = calls[2][:3]
    assert k < olay.cap_items
    olay.put(oraw, 0, np.array([1.0], np.float32), at_item=olay.cap_items - 1)
    s.judge(calls, exact=True)


@pytest.mark.parametrize("kind", KINDS)
def test_one_interior_output_left_as_poison(streams, kind):
    s = streams[kind]
    calls = s.device()
    oraw, olay, k = calls[2][:3]
    olay.put(oraw, 0, np.array([sc.POISON], np.uint32), at_item=k // 2)
    with pytest.raises(sc.WrittenError, match="never stored"):
        s.judge(calls, exact=True)


def test_half_of_a_complex_sample_left_as_poison():
    lay = sc.out_layout(1, 8, 10)
    raw = lay.poisoned()
    lay.put(raw, 0, np.arange(1, 21, dtype=np.float32))
    sc.check_written(raw, lay, 10)
    lay.put(raw, 0, np.array([sc.POISON], np.uint32).view(np.float32), at_item=3)       # the real part of sample 3
    with pytest.raises(sc.WrittenError, match="item 3"):
        sc.check_written(raw, lay, 10)


def test_a_tx10_group_left_as_poison_and_a_byte_past_the_groups():
    lay = sc.out_layout(2, 5, 7, gran=5)
    raw = lay.poisoned()
    for c in range(2):
        lay.put(raw, c, np.arange(35, dtype=np.uint8))
    sc.check_written(raw, lay, 7)
    bad = raw.copy()
    g = slice(lay.start(1) + 10, lay.start(1) + 15)
    bad.view(np.uint8)[g] = lay.poisoned().view(np.uint8)[g]
    with pytest.raises(sc.WrittenError, match="never stored"):
        sc.check_written(bad, lay, 7)
    bad = raw.copy()
    bad.view(np.uint8)[lay.start(0) + 35] ^= 0xFF
    with pytest.raises(sc.WrittenError, match="gap after channel 0"):
        sc.check_written(bad, lay, 7)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("exact", [True, False])
def test_input_became_zeros(streams, orc, kind, exact):
    """The reference computed from x, the result computed from zeros."""
    s = streams[kind]
    calls = s.device(x=np.zeros_like(s.x), orc=orc)
    with pytest.raises(sc.ValuesError):
        s.judge(calls, exact=exact)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("where", ["a sample", "the lead", "a stride gap", "the tail"])
def test_one_input_word_changed_after_the_call(streams, kind, where):
    s = streams[kind]
    calls = s.device()
    ilay = sc.in_layout(NCH, 4, CUTS[3] - CUTS[2])
    word = {"a sample": ilay.start(1) // 4 + 17, "the lead": 3, "a stride gap": (ilay.start(0) + ilay.cap) // 4 + 1,
            "the tail": ilay.words - 1}[where]
    after = calls[2][3]
    assert after.size == ilay.words
    after[word] = 0
    with pytest.raises(sc.InputError):
        s.judge(calls, exact=True)


def test_everything_outside_the_samples_is_nan_in_a_laid_out_input():
    x = np.stack([synth.synth_f32(100, ch=c) for c in range(3)])
    for aligned in (True, False):
        lay, raw = sc._lay_input(x, 3, 4, 10, 60, aligned)
        f = raw.view(np.float32)
        own = np.zeros(raw.size, bool)
        for c in range(3):
            o = lay.start(c) // 4
            assert (lay.start(c) % 16 == 0) == aligned
            assert np.array_equal(f[o:o + 50], x[c, 10:60])
            own[o:o + 50] = True
        assert np.isnan(f[~own]).all() and (raw[~own] == sc.POISON).all()
        assert own[0] == False and own[-1] == False and lay.stride_items > 50          # noqa: E712


def test_one_sample_of_250001_off_by_a_tenth_of_a_percent(orc):
    """Passes the rel-RMS gate (about 1e-6 against 1e-5); the per-sample gate sees it."""
    taps = synth.taps_cfg1()                                      # 63 taps
    n = 250003
    x = synth.synth_f32(n, ch=3)
    ref = orc.Resample(taps, 1, B).stream(x, 1.0)[0][:250001]
    A = orc.Resample(np.abs(taps), 1, B).stream(np.abs(x), 1.0)[0][:250001]
    assert ref.size == 250001
    bound = sc.direct_bound(A, 63)
    j = int(np.argsort(np.abs(ref))[ref.size // 2])               # a sample of typical size
    got = ref.copy()
    got[j] = np.float32(got[j] * np.float32(1.001))
    assert sc.rel_rms(got, ref) < 2e-6                            # five times under the rel-RMS gate
    assert sc.check_values(got, ref) == 0.0                       # the rel-RMS gate alone lets it through
    with pytest.raises(sc.ValuesError) as e:
        sc.check_values(got, ref, bound=bound)
    assert e.value.gate == "sample"
    zeroed = ref.copy()
    zeroed[int(np.argmax(np.abs(ref)))] = 0.0
    with pytest.raises(sc.ValuesError):
        sc.check_values(zeroed, ref, bound=bound)


# ------------------------------------------------------------------------------ the bounds are not too tight
# (taps, U, rate, blksize, n): the shapes of tests/test_gpu_stream_guarded.py
def _shapes():
    rng = np.random.default_rng(11)
    return {
        "5/3 x 381": (synth.taps_cfg3(), 3, 5.0 / 3.0, B, 8000),
        "5/3 x 381 short": (synth.taps_cfg3(), 3, 5.0 / 3.0, B, 2000),
        "/8 x 64": (synth.taps_cfg4(), 1, 8.0, B, 8003),
        "x3": (synth.lowpass_taps(95, 0.15, gain=3.0), 3, 1.0 / 3.0, B, 3000),
        "/63": (synth.lowpass_taps(505, 0.9 / 63.0), 1, 63.0, B, 9010),
        "10/9": (synth.lowpass_taps(271, 0.045, gain=9.0), 9, 10.0 / 9.0, B, 5000),
        "1.77 B 256": (synth.taps_cfg3(), 3, 1.77, 256, 256 * 5 + 85),
        "0.77 B 256": (synth.taps_cfg3(), 3, 0.77, 256, 256 * 5 + 85),
        "1.77 B 4096": (synth.taps_cfg3(), 3, 1.77, B, B * 5 + 1365),
        "0.77 B 4096": (synth.taps_cfg3(), 3, 0.77, B, B * 5 + 1365),
        "random taps": (rng.standard_normal(5 * 4).astype(np.float32), 4, 2.31, 1000, 7001),
    }


@pytest.mark.parametrize("name", list(_shapes()))
def test_the_float32_oracle_sits_inside_the_direct_sum_bound(orc, name):
    """The float32 oracle against the float64 direct sum at the law's own (position, mu) sequence: inside HALF the bound
    the GPU tests use (which is for two float32 results), on every shape they use.  Also: the numpy replay of the time law
    reproduces the oracle's counts call by call."""
    taps, Up, rate, blk, n = _shapes()[name]
    rate = float(np.float32(rate))
    x = synth.synth_f32(n, ch=9)
    cuts = sorted({0, 1, min(blk, n), n})
    got, counts = sc.reference_stream(orc.Resample(taps, Up, blk), x, rate, cuts, blk)
    pos, mu, law_counts, _ = sc.law_positions(n, Up, rate, cuts, blk)
    assert counts == law_counts
    ref = sc.direct_resample64(x, taps, Up, pos, mu)
    A = sc.direct_resample64(np.abs(x), np.abs(taps), Up, pos, mu)
    L = -(-len(taps) // Up)
    worst = float(np.max(np.abs(got - ref) / (0.5 * sc.direct_bound(A, L))))
    print("%s: L %d, oracle at %.2f x 2^-24 A worst, %.3f of half the bound" % (name, L, float(np.max(np.abs(got - ref) / (sc.U24 * A + 1e-30))), worst))
    assert worst <= 1.0
    A32 = sc.reference_stream(orc.Resample(np.abs(taps), Up, blk), np.abs(x), rate, cuts, blk)[0]
    assert np.all(np.abs(got - ref) <= 0.5 * sc.direct_bound(A32, L) * (1 + 1e-5))        # A from the oracle serves as well


def _overlap_save_c64(x, h, N):
    """y = x * h by overlap-save with N-point transforms in float32 (scipy.fft keeps complex64)."""
    import scipy.fft
    x, h = np.asarray(x, np.complex64), np.asarray(h, np.complex64)
    ovl = len(h) - 1
    adv = N - ovl
    H = scipy.fft.fft(np.concatenate([h, np.zeros(N - len(h), np.complex64)]))
    assert H.dtype == np.complex64
    xp = np.concatenate([np.zeros(ovl, np.complex64), x, np.zeros(N, np.complex64)])
    y = np.empty(len(x), np.complex64)
    for b in range(0, len(x), adv):
        seg = scipy.fft.ifft(scipy.fft.fft(xp[b:b + N]) * H)
        m = min(adv, len(x) - b)
        y[b:b + m] = seg[ovl:ovl + m]
    return y


@pytest.mark.parametrize("name, N, window", [("fir 256", 4096, 4096), ("fir 3841 partition", 4096, 4096), ("phase of 381", 4096, 4096),
                                             ("component of 5/3 x 381", 256, 256)])
def test_float32_overlap_save_sits_inside_the_transform_bound(name, N, window):
    h = {"fir 256": synth.taps_cfg2(), "fir 3841 partition": synth.lowpass_taps(3841, 0.1)[:2561],
         "phase of 381": synth.taps_cfg3()[0::3], "component of 5/3 x 381": synth.taps_cfg3()[0::3][0::5]}[name]
    n = 3 * N + 17
    xi = synth.synth_cf32(n, ch=21)
    x = xi[0::2] + 1j * xi[1::2]
    x[N:N + 500] *= 1e-3                                   # a quiet passage: the bound follows the window's energy
    got = _overlap_save_c64(x, h, N)
    ref = np.convolve(x.astype(np.complex128), h.astype(np.float64))[:n]
    xi = np.ascontiguousarray(x.astype(np.complex64)).view(np.float32)
    bound = sc.transform_bound(xi, h, N, window, np.arange(n), cplx=True)
    worst = float(np.max(np.abs(got - ref) / bound[0::2]))
    print("%s: N %d, float32 overlap-save at %.4f of the bound" % (name, N, worst))
    assert worst <= 1.0


def test_the_guarded_gpu_streams_end_with_and_without_a_pending_leftover():
    """tests/test_gpu_stream_guarded.py chooses its stream lengths so that each family ends both ways"""
    import test_gpu_stream_guarded as g
    ends = {k: sc.closed_form_total(n, Up, S) * S - n * Up == -1 for k, (_, Up, S, n) in g.INT_SHAPES.items()}
    assert set(ends.values()) == {True, False}, ends
    gen = {(rate, blk, cuts[-1]): sc.law_positions(cuts[-1], g.GEN_U, float(np.float32(rate)), cuts, blk)[3] for rate, blk, cuts in g.GEN_STREAMS}
    print(ends, gen)
    assert set(gen.values()) == {True, False}, gen
