"""The burst demodulator (sfe_dsp_burst_*) on the GPU: its estimates against the float64 plan within bars that a float32
numpy restatement of the law sets on the CPU, its symbols against the plan run with the device's own estimates, the six
contracts about bits checked literally, the chain behind a real correlator handle, and process_stream's refusals."""
import ctypes as C

import numpy as np
import pytest

from simplefe_amd import synth

pytestmark = pytest.mark.gpu
F32 = np.float32
SENT = np.float32(-7654.25)
# (sps, N, Lp, lag); the reach of the last one, 16392 samples, is above the LDS threshold: it is read from global memory twice
SHAPES = [(4, 32, 8, 1), (10, 256, 32, 4), (50, 64, 16, 2), (64, 16, 4, 1), (4, 4096, 64, 8)]
SHAPE_IDS = ["sps%d-N%d-Lp%d-lag%d" % s for s in SHAPES]
PAYLOAD = [0, 1, 5, 6, 4]          # tests/test_burst_host.py: the payloads that do not slip a symbol at tau = -0.49 sps
# Per record field (tau samples, f turns per symbol, theta turns, a relative, q, evm): 8 times the worst deviation of law32
# below -- the law in float32 numpy, float32 sums -- from the float64 plan over synth.burst_cases of the five shapes,
# measured on the CPU (measure_bars(); DESIGN.md 4.16 quotes them).  The factor covers the device's other order of
# summation and its atan2f.  Nothing here comes from the device's output.
BARS = tuple(8 * w for w in (1.91e-6, 2.99e-8, 1.50e-7, 1.40e-7, 2.39e-7, 6.18e-9))
EVM_BAR = 2 * 3.45e-2               # twice the plan's worst symbol EVM at (4, 32, 8, 1): tests/test_burst_host.py, DESIGN.md 4.16


@pytest.fixture(scope="module")
def api():
    from simplefe_amd import api as a
    return a


@pytest.fixture(scope="module")
def L():
    from simplefe_amd import lib
    return lib


@pytest.fixture(scope="module")
def hip():
    h = C.CDLL("libamdhip64.so")
    for name, args in (("hipStreamCreate", [C.POINTER(C.c_void_p)]), ("hipStreamBeginCapture", [C.c_void_p, C.c_int]),
                       ("hipStreamEndCapture", [C.c_void_p, C.POINTER(C.c_void_p)]), ("hipGraphDestroy", [C.c_void_p]),
                       ("hipStreamDestroy", [C.c_void_p]), ("hipGraphGetNodes", [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)])):
        fn = getattr(h, name)
        fn.argtypes, fn.restype = args, C.c_int
    return h


def _bits(y):
    return np.ascontiguousarray(y).view(np.uint32)


_packed = {}


def packed_cases(shape):
    """synth.burst_cases of a shape laid end to end in one stream: (x complex64, idx uint32 per burst, the cases)."""
    if shape not in _packed:
        sps, N, Lp, lag = shape
        cs = synth.burst_cases(sps, N, lag, seed=synth.SEED + PAYLOAD[SHAPES.index(shape)])
        n = cs[0][0].size
        _packed[shape] = (np.concatenate([c[0] for c in cs]), np.array([i * n + c[1] for i, c in enumerate(cs)], np.uint32), cs)
    return _packed[shape]


def law32(x, o, pre, sps, N, lag):
    """The law of include/sfe_dsp.h on one burst in float32 numpy -- the same steps, float32 sums (numpy's order), the turn
    count alone in float64 -- as float32[6]: tau, f, theta, a, q, evm."""
    x, pre = np.asarray(x, np.complex64), np.asarray(pre, np.complex64)
    Lp, two_pi = pre.size, F32(6.2831855)
    E_p = F32((pre.real.astype(np.float64) ** 2 + pre.imag.astype(np.float64) ** 2).sum())
    r = np.arange(sps)
    w = np.exp(-2j * np.pi * r / sps).astype(np.complex64)
    i = np.arange(N * sps)
    v = x[o + i]
    c = ((v.real * v.real + v.imag * v.imag) * w[i % sps]).sum(dtype=np.complex64)
    tau = F32(0) - F32(sps) * (np.arctan2(c.imag, c.real) / two_pi)
    if tau <= F32(-0.5 * sps):
        tau = tau + F32(sps)
    m = int(np.floor(tau))
    mu, one, two = F32(tau - F32(m)), F32(1), F32(2)
    lag4 = [-mu * (mu - one) * (mu - two) / F32(6), (mu + one) * (mu - one) * (mu - two) / two, -(mu + one) * mu * (mu - two) / two,
            (mu + one) * mu * (mu - one) / F32(6)]
    at = o + np.arange(N) * sps + m - 1
    y = np.zeros(N, np.complex64)
    for q in range(4):
        y = y + lag4[q] * x[at + q]
    z = y[:Lp] * np.conj(pre)
    R = (z[lag:] * np.conj(z[:-lag])).sum(dtype=np.complex64)
    f = F32(np.arctan2(R.imag, R.real) / (two_pi * F32(lag)))

    def unturn(t):
        t = (t - np.rint(t)).astype(F32)
        return (np.cos(two_pi * t) - 1j * np.sin(two_pi * t)).astype(np.complex64)

    k = np.arange(N, dtype=np.float64)
    S = (z * unturn(np.float64(f) * k[:Lp])).sum(dtype=np.complex64)
    S2 = F32(S.real * S.real + S.imag * S.imag)
    theta, a = F32(np.arctan2(S.imag, S.real) / two_pi), F32(np.sqrt(S2) / E_p)
    sym = (y * unturn(np.float64(theta) + np.float64(f) * k) / a).astype(np.complex64)
    ey = (y[:Lp].real ** 2 + y[:Lp].imag ** 2).sum(dtype=F32)
    d = sym[:Lp] - pre
    return np.array([tau, f, theta, a, S2 / (E_p * ey), (d.real ** 2 + d.imag ** 2).sum(dtype=F32) / E_p], F32)


def field_errors(rec, want):
    """|rec - want| per field of (n, 8) records against the plan's: theta around the circle, a relative."""
    e = np.abs(rec[:, :6].astype(np.float64) - want[:, :6])
    t = e[:, 2]
    e[:, 2] = np.minimum(t, np.abs(1.0 - t))
    e[:, 3] /= want[:, 3]
    return e


def measure_bars(api):
    """CPU only: the worst deviation of law32 from the float64 plan per field over the cases of every shape."""
    worst = np.zeros(6)
    for shape in SHAPES:
        sps, N, Lp, lag = shape
        x, idx, cs = packed_cases(shape)
        for b, c in enumerate(cs):
            pre = c[2][:Lp].astype(np.complex64)
            want = api.burst_plan(pre, sps, N, lag, x=x, start_base=int(idx[b]))[1].astype(np.float64)
            got = law32(x, int(idx[b]), pre, sps, N, lag)[None, :]
            worst = np.maximum(worst, field_errors(got, want).max(axis=0))
    return worst


def _rel_rms(got, want):
    want = np.asarray(want, np.complex128)
    return float(np.sqrt((np.abs(np.asarray(got, np.complex128) - want) ** 2).sum() / (np.abs(want) ** 2).sum()))


def stream_of(sps, n, seed, u8=False):
    """A continuous shaped QPSK stream of n samples with a little carrier on it: every window of it is a burst of sorts."""
    a = synth.psk_symbols(n // sps + 2, 4, seed=synth.SEED + seed)
    x = synth.burst_signal(a, sps, n, 0, 0.37, 0.013, 0.5, 0.6)
    if not u8:
        return x
    b = np.clip(np.rint(x.view(F32).astype(np.float64) * 127.0 + 128.0), 0, 255).astype(np.uint8)
    return b


def preamble_of(sps, Lp, seed):
    return synth.psk_symbols(Lp + 2, 4, seed=synth.SEED + seed)[:Lp].astype(np.complex64)


# the two BPSK / QPSK payloads of a shape share their first symbols only by chance: each case brings its own preamble, so the
# estimate tests run one handle per modulation
def _by_preamble(cs, Lp):
    groups = {}
    for b, c in enumerate(cs):
        groups.setdefault(c[2][:Lp].astype(np.complex64).tobytes(), []).append(b)
    return [(np.frombuffer(k, np.complex64), v) for k, v in groups.items()]


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_estimates_and_symbols_against_the_float64_plan(api, shape):
    sps, N, Lp, lag = shape
    x, idx, cs = packed_cases(shape)
    for pre, which in _by_preamble(cs, Lp):
        ix = idx[which]
        h = api.Burst(pre, sps, N, lag)
        sym, rec, st = (v[0] for v in h.demodulate(x, idx=ix))
        h.close()
        assert not st.any(), st
        psym, prec, pst = api.burst_plan(pre, sps, N, lag, x=x, idx=ix)
        err = field_errors(rec, prec.astype(np.float64)).max(axis=0)
        print("record |diff| per field", " ".join("%.2e" % e for e in err), "of bars", " ".join("%.2e" % b for b in BARS))
        assert (err <= np.array(BARS)).all(), err
        assert not _bits(rec[:, 6:]).any()
        # the symbol path alone: the plan with the device's own estimates
        gsym, grec, gst = api.burst_plan(pre, sps, N, lag, x=x, idx=ix, given=rec)
        worst = max(_rel_rms(sym[b], gsym[b]) for b in range(len(which)))
        print("symbols rel-RMS against the plan given the device's estimates: %.2e" % worst)
        assert not gst.any() and worst <= 1e-5


class Run:
    """One call's buffers with room around every output: the input rows `lead` samples into their buffer, outputs with
    strides wider than their payload, a sentinel everywhere else."""

    def __init__(self, api, h, x, n_bursts, idx=None, gate=None, out_pad=0, st_pad=0, lead=0, in_pad=0, start_base=0, start_step=0):
        self.api, S, N = api, h.n_streams, h.n_sym
        x = np.asarray(x).reshape(S, -1)
        self.u8 = x.dtype == np.uint8
        w = 1 if self.u8 else 2                         # items of the host array per sample / 2
        n_in = x.shape[1] // 2 if self.u8 else x.shape[1]
        row = x if self.u8 else x.astype(np.complex64).view(F32)
        self.in_stride = n_in + in_pad
        fill = 0x55 if self.u8 else np.nan
        buf = np.full(2 * lead + S * self.in_stride * 2 + 8, fill, row.dtype)
        for s in range(S):
            buf[2 * lead + s * self.in_stride * 2:][:n_in * 2] = row[s]
        self.d_in = api.DeviceArray.from_bytes(buf) if self.u8 else api.DeviceArray.from_numpy(buf)
        self.in_ptr = self.d_in.ptr + lead * (2 if self.u8 else 8)
        self.nb, self.out_stride, self.st_stride = n_bursts, N + out_pad, n_bursts + st_pad
        self.held = [self.d_in]
        self.d_idx = self.d_gate = None
        if idx is not None:
            self.d_idx = api.DeviceArray.from_numpy(np.ascontiguousarray(idx, np.uint32).reshape(S, n_bursts).view(F32))
            self.held.append(self.d_idx)
        if gate is not None:
            self.d_gate = api.DeviceArray.from_numpy(np.ascontiguousarray(gate, F32).reshape(S, n_bursts))
            self.held.append(self.d_gate)
        self.sizes = (4 + S * n_bursts * self.out_stride * 2 + 6, 3 + S * n_bursts * 8 + 5, 5 + S * self.st_stride + 3)
        self.lead = (4, 3, 5)                            # floats before each output's first slot (out stays 8-byte aligned)
        self.d = [api.DeviceArray.from_numpy(np.full(n, SENT, F32)) for n in self.sizes]
        self.held += self.d
        self.k = h.process_stream(self.in_ptr, n_in, n_bursts, self.d[0].ptr + 4 * self.lead[0], self.d_idx, self.d_gate,
                                  self.d[1].ptr + 4 * self.lead[1], self.d[2].ptr + 4 * self.lead[2], start_base, start_step,
                                  in_stride=self.in_stride, out_stride=self.out_stride, status_stride=self.st_stride)
        api.sync()

    def free(self):
        for d in self.held:
            d.free()


def run(api, h, x, n_bursts, **kw):
    """Run one call through guarded buffers: (symbols, records, statuses), the guard bands checked."""
    S, N = h.n_streams, h.n_sym
    r = Run(api, h, x, n_bursts, **kw)
    try:
        assert r.k == n_bursts
        raw = [d.to_numpy() for d in r.d]
    finally:
        r.free()
    sent = _bits(np.array([SENT]))[0]
    out = raw[0][r.lead[0]:r.lead[0] + S * n_bursts * r.out_stride * 2].reshape(S * n_bursts, r.out_stride * 2)
    rec = raw[1][r.lead[1]:r.lead[1] + S * n_bursts * 8].reshape(S, n_bursts, 8)
    st = raw[2][r.lead[2]:r.lead[2] + S * r.st_stride].reshape(S, r.st_stride)
    assert (_bits(raw[0][:r.lead[0]]) == sent).all() and (_bits(raw[0][r.lead[0] + S * n_bursts * r.out_stride * 2:]) == sent).all()
    assert (_bits(out[:, 2 * N:]) == sent).all()
    assert (_bits(raw[1][:r.lead[1]]) == sent).all() and (_bits(raw[1][r.lead[1] + S * n_bursts * 8:]) == sent).all()
    assert (_bits(raw[2][:r.lead[2]]) == sent).all() and (_bits(raw[2][r.lead[2] + S * r.st_stride:]) == sent).all()
    assert (_bits(st[:, n_bursts:]) == sent).all()
    sym = np.ascontiguousarray(out[:, :2 * N]).view(np.complex64).reshape(S, n_bursts, N)
    return sym, rec, np.ascontiguousarray(st[:, :n_bursts]).view(np.int32)


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[4]], ids=[SHAPE_IDS[1], SHAPE_IDS[4]])
@pytest.mark.parametrize("n_streams,n_bursts", [(1, 1), (1, 3), (2, 70)])
def test_runs_repeat_and_a_burst_depends_on_its_reach_alone(api, shape, n_streams, n_bursts):
    """Contracts 1, 2 and 6: the same call twice; every burst of the call against a one-burst call of a one-stream handle at
    another input address, output address and stride, without an index table; windows 37 samples apart overlap."""
    sps, N, Lp, lag = shape
    reach, step = (N + 2) * sps, 37
    n = reach + (n_bursts - 1) * step + 9
    x = np.stack([stream_of(sps, n, 11 + s) for s in range(n_streams)])
    pre = preamble_of(sps, Lp, 3)
    rng = np.random.default_rng(5)
    jit = rng.integers(0, 9, size=(n_streams, n_bursts)).astype(np.uint32)          # o = sps + b step + jitter
    h = api.Burst(pre, sps, N, lag, n_streams=n_streams)
    a = run(api, h, x, n_bursts, idx=jit, start_base=sps, start_step=step, out_pad=3, st_pad=2, lead=1, in_pad=5)
    b = run(api, h, x, n_bursts, idx=jit, start_base=sps, start_step=step, out_pad=3, st_pad=2, lead=1, in_pad=5)
    h.close()
    assert not a[2].any()
    for u, v in zip(a, b):
        assert np.array_equal(_bits(u), _bits(v))
    one = api.Burst(pre, sps, N, lag)
    for s in range(n_streams):
        for bi in range(n_bursts):
            o = sps + bi * step + int(jit[s, bi])
            cut = o - sps - (bi % 3)                    # the one-burst call sees the stream from here on, up to the reach's end
            got = run(api, one, x[s, cut:o + (N + 1) * sps], 1, start_base=o - cut, out_pad=bi % 5, lead=2 + bi % 4)
            for u, v in zip(a, got):
                assert np.array_equal(_bits(u[s, bi]), _bits(v[0, 0])), (s, bi)
    one.close()


# two shapes beside the issue's, for the launches that ask for more than 64 KB of dynamic LDS: (10, 1024, 32, 4) stages its
# reach (9 024 + 90 288 = 99 312 bytes), (4, 4096, 4096, 8) does not and still needs 66 112 for y, z and the tables
OVER_64K = [(10, 1024, 32, 4), (4, 4096, 4096, 8)]
U8_SHAPES = [SHAPES[0], SHAPES[4]] + OVER_64K


@pytest.mark.parametrize("shape", U8_SHAPES, ids=["sps%d-N%d-Lp%d-lag%d" % s for s in U8_SHAPES])
def test_u8_input_gives_the_bits_of_the_converted_samples(api, L, shape):
    """Contract 3, with the bytes at an address that is 2 mod 4; and both instantiations' symbols against the plan."""
    sps, N, Lp, lag = shape
    n_bursts, step = 3, 21
    n = (N + 2) * sps + (n_bursts - 1) * step
    by = stream_of(sps, n, 21, u8=True)
    pre = preamble_of(sps, Lp, 4)
    h = api.Burst(pre, sps, N, lag)
    want = run(api, h, synth.u8_to_cf32(by), n_bursts, start_base=sps, start_step=step)
    h.set_input_format(L.FMT_U8)
    got = run(api, h, by, n_bursts, start_base=sps, start_step=step, lead=1)
    h.close()
    assert not want[2].any()
    for u, v in zip(want, got):
        assert np.array_equal(_bits(u), _bits(v))
    psym, prec, pst = api.burst_plan(pre, sps, N, lag, x=synth.u8_to_cf32(by), n_bursts=n_bursts, start_base=sps, start_step=step, given=want[1][0])
    assert not pst.any() and max(_rel_rms(want[0][0, b], psym[b]) for b in range(n_bursts)) <= 1e-5


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_the_constant_case_is_exact(api, shape):
    """Contract 4: timing_mode 1, p all ones, x = 1+0j: f = theta = +0, a = q = 1, evm = 0, y^ exactly 1+0j."""
    sps, N, Lp, lag = shape
    h = api.Burst(np.ones(Lp), sps, N, lag, timing_mode=1)
    sym, rec, st = run(api, h, np.ones((N + 2) * sps + 2, np.complex64), 3, start_base=sps, start_step=1)
    h.close()
    assert not st.any()
    assert np.array_equal(_bits(sym), _bits(np.ones((1, 3, N), np.complex64)))
    assert np.array_equal(_bits(rec), _bits(np.tile(np.array([0, 0, 0, 1, 1, 0, 0, 0], F32), (1, 3, 1))))


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[4]], ids=[SHAPE_IDS[1], SHAPE_IDS[4]])
def test_failed_bursts_get_the_stated_bits_and_leave_their_neighbours_alone(api, shape):
    """Contract 5: of seven bursts one holds a NaN sample, one an infinite one (timing fixed: only the finite check can see
    it), one is gated, one has a NaN gate and one starts before the buffer; the rest equal a call without any of that."""
    sps, N, Lp, lag = shape
    nb, step = 7, (N + 2) * sps + 3                     # windows that do not overlap: a bad sample spoils one burst only
    n = nb * step + sps
    x = stream_of(sps, n, 31)
    pre = preamble_of(sps, Lp, 6)
    qnan = np.array([np.nan, np.nan, np.nan, np.nan, np.nan, np.nan, 0, 0], F32)
    for mode in (0, 1):
        h = api.Burst(pre, sps, N, lag, timing_mode=mode, min_gate=0.5)
        clean = run(api, h, x, nb, start_base=sps, start_step=step)
        bad = x.copy()
        bad[1 * step] = complex(np.nan, 0.0)            # burst 1: the first sample of its reach
        bad[3 * step + (N + 2) * sps - 1] = complex(0.0, np.inf)         # burst 3: the last one
        gate = np.array([1, 1, 0.25, 1, np.nan, 1, 0.5], F32)
        idx = np.zeros(nb, np.uint32)
        idx[5] = 2 ** 32 - 5 * step - sps - 1           # burst 5 starts at o = 2^32 - 1: far beyond the buffer
        sym, rec, st = run(api, h, bad, nb, idx=idx, gate=gate, start_base=sps, start_step=step)
        h.close()
        assert not clean[2].any() and st[0].tolist() == [0, 1, 2, 1, 2, 3, 0]
        for b in range(nb):
            if st[0, b]:
                assert not _bits(sym[0, b]).any()
                assert np.isnan(rec[0, b, :6]).all() and ((_bits(rec[0, b, :6]) & 0x7fc00000) == 0x7fc00000).all() and not _bits(rec[0, b, 6:]).any()
            else:
                assert np.array_equal(_bits(sym[0, b]), _bits(clean[0][0, b])) and np.array_equal(_bits(rec[0, b]), _bits(clean[1][0, b]))
    # the range's two edges: a reach that ends exactly at n_in or begins exactly at 0 is in, one sample more is out
    h = api.Burst(pre, sps, N, lag)
    reach = (N + 2) * sps
    assert run(api, h, x[:reach], 1, start_base=sps)[2].tolist() == [[0]]
    assert run(api, h, x[:reach], 2, start_base=sps - 1, start_step=2)[2].tolist() == [[3, 3]]
    assert run(api, h, x[:reach + 1], 2, start_base=sps, start_step=1)[2].tolist() == [[0, 0]]
    assert run(api, h, x[:reach], 1, start_base=-2 ** 40)[2].tolist() == [[3]]
    h.close()


def test_the_chain_behind_a_correlator_stays_on_the_device(api):
    """A real correlator handle (L = 13, K = 1, B = V) finds two bursts in blocks 1 and 3 of five; its peak tables go to the
    demodulator as they lie on the device; the other blocks are gated off; the symbols are the transmitted ones."""
    sps, N, Lp, lag = SHAPES[0]
    Lc, B = 13, api.corr_plan(13, 1, 3840)[0]
    assert B == 3840
    a = synth.psk_symbols(N, 4, seed=synth.SEED + 77)
    tpl = synth.burst_signal(a, sps, (N + 40) * sps, 32, 0.0)[32:32 + Lc]              # the burst's first 13 samples, from symbol 0's peak
    x = np.zeros(5 * B, np.complex64)
    where = {1: (B + 500, 0.3, 0.004, 1.1, 0.8), 3: (3 * B + 1717, -0.2, -0.006, -2.0, 1.7)}     # block: o, tau, f, phase, amp
    for o, tau, f, phase, amp in where.values():
        x += synth.burst_signal(a, sps, x.size, o, tau, f, phase, amp)
    corr = api.Corr(tpl, B, min_energy=0.5)
    h = api.Burst(a[:Lp], sps, N, lag, min_gate=0.5)
    d_x = api.DeviceArray.from_numpy(x.view(F32))
    d_val, d_idx = api.DeviceArray(5), api.DeviceArray(5)
    d_out, d_rec, d_st = api.DeviceArray(5 * N * 2), api.DeviceArray(5 * 8), api.DeviceArray(5)
    try:
        assert corr.process_stream(d_x, x.size, d_val, d_idx) == 5
        assert h.process_stream(d_x, x.size, 5, d_out, d_idx, d_val, d_rec, d_st, start_base=-(Lc - 1), start_step=B) == 5
        api.sync()
        sym = d_out.to_numpy().view(np.complex64).reshape(5, N)
        st, idx, val = d_st.to_numpy().view(np.int32), d_idx.to_numpy().view(np.uint32), d_val.to_numpy()
    finally:
        for d in (d_x, d_val, d_idx, d_out, d_rec, d_st):
            d.free()
        corr.close()
        h.close()
    print("peaks", val, idx, "statuses", st)
    assert st.tolist() == [2, 0, 2, 0, 2]
    for j, (o, *_) in where.items():
        assert j * B + int(idx[j]) - (Lc - 1) == o
        evm = _rel_rms(sym[j], a)
        print("block %d: EVM %.3e of %.3e" % (j, evm, EVM_BAR))
        assert evm <= EVM_BAR
    assert not _bits(sym[[0, 2, 4]]).any()


def test_refusals_launch_nothing(api, L, hip):
    sps, N, Lp, lag = SHAPES[0]
    S, nb = 2, 3
    n = (N + 2) * sps + 8
    x = np.stack([stream_of(sps, n, 41), stream_of(sps, n, 42)])
    h = api.Burst(preamble_of(sps, Lp, 7), sps, N, lag, n_streams=S)
    d_in = api.DeviceArray.from_numpy(np.concatenate([x.view(F32).ravel(), np.zeros(64, F32)]))
    d_idx, d_gate = api.DeviceArray.from_numpy(np.zeros(S * nb + 8, F32)), api.DeviceArray.from_numpy(np.ones(S * nb + 8, F32))
    sentinel = np.full(S * nb * N * 2 + 64, SENT, F32)
    d_out, d_rec, d_st = (api.DeviceArray.from_numpy(sentinel) for _ in range(3))
    lib = L.load()
    k = C.c_size_t(7)

    def call(pi=d_in.ptr, n_in=n, in_stride=n, px=d_idx.ptr, pg=d_gate.ptr, n_bursts=nb, po=d_out.ptr, ostride=N, pr=d_rec.ptr, ps=d_st.ptr,
             sstride=nb, stream=None, hh=None, base=sps, step=2):
        return lib.sfe_dsp_burst_process_stream(hh or h._h, pi, n_in, in_stride, px, nb, pg, nb, n_bursts, base, step, po, ostride, pr, ps, sstride,
                                                C.byref(k), stream)

    assert call(ostride=N - 1) == L.SFE_ERANGE                       # a burst's symbols one short
    assert call(sstride=nb - 1) == L.SFE_ERANGE
    assert call(pi=None) == L.SFE_EINVAL and call(po=None) == L.SFE_EINVAL
    assert call(pi=d_in.ptr + 4) == L.SFE_EINVAL                     # misaligned, each of the six
    assert call(po=d_out.ptr + 4) == L.SFE_EINVAL
    assert call(px=d_idx.ptr + 2) == L.SFE_EINVAL
    assert call(pg=d_gate.ptr + 1) == L.SFE_EINVAL
    assert call(pr=d_rec.ptr + 2) == L.SFE_EINVAL
    assert call(ps=d_st.ptr + 3) == L.SFE_EINVAL
    assert call(in_stride=n - 1) == L.SFE_EINVAL                     # two streams whose rows overlap
    assert call(n_in=1 << 31, in_stride=1 << 31) == L.SFE_EINVAL
    assert call(n_bursts=1 << 30, sstride=1 << 30) == L.SFE_EINVAL   # n_streams n_bursts = 2^31
    for base, step in ((2 ** 63 - 1, 0), (-2 ** 63, 0), (0, 2 ** 62), (0, -2 ** 62)):          # starts that leave int64
        assert call(base=base, step=step) == L.SFE_EINVAL
    assert call(ostride=1 << 60) == L.SFE_EINVAL and call(in_stride=1 << 61) == L.SFE_EINVAL     # byte ranges that reach 2^62
    assert call(sstride=1 << 61) == L.SFE_EINVAL
    assert call(po=d_in.ptr + 8 * (2 * n - 1)) == L.SFE_EINVAL       # each output over the input, the index and the gate table
    assert call(pr=d_in.ptr) == L.SFE_EINVAL
    assert call(ps=d_in.ptr + 16) == L.SFE_EINVAL
    assert call(po=d_idx.ptr) == L.SFE_EINVAL and call(pr=d_idx.ptr + 4) == L.SFE_EINVAL and call(ps=d_idx.ptr + 4 * (S * nb - 1)) == L.SFE_EINVAL
    assert call(po=d_gate.ptr) == L.SFE_EINVAL and call(pr=d_gate.ptr) == L.SFE_EINVAL and call(ps=d_gate.ptr) == L.SFE_EINVAL
    assert call(pr=d_out.ptr + 8) == L.SFE_EINVAL                    # two outputs over one another
    assert call(ps=d_out.ptr + 4 * (S * nb * N * 2 - 1)) == L.SFE_EINVAL
    assert call(ps=d_rec.ptr + 4) == L.SFE_EINVAL
    assert lib.sfe_dsp_burst_process_stream(h._h, d_in.ptr, n, n, None, 0, None, 0, nb, sps, 2, d_out.ptr, N, None, None, 0, None, None) == L.SFE_EINVAL
    assert k.value == 0
    assert call(n_bursts=0) == L.SFE_OK and k.value == 0             # no bursts: a no-op
    # a capturing stream: the call is refused, and the capture ends as an empty graph
    s = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(s)) == 0
    assert hip.hipStreamBeginCapture(s, 2) == 0            # relaxed mode: the refused call launches nothing
    try:
        rc = call(stream=s.value)
        msg = lib.sfe_dsp_last_error()
    finally:
        g = C.c_void_p()
        ended = hip.hipStreamEndCapture(s, C.byref(g))
    nodes = C.c_size_t(0)
    if g.value:
        assert hip.hipGraphGetNodes(g, None, C.byref(nodes)) == 0
        hip.hipGraphDestroy(g)
    hip.hipStreamDestroy(s)
    assert rc == L.SFE_ESTATE and k.value == 0 and b"graph capture is not supported" in msg
    assert ended == 0 and (not g.value or nodes.value == 0)
    # a live handle of another block is refused by every burst function, and burst's destroy frees nothing of it
    other = api.Corr(np.ones(13, np.complex64), 3840)
    assert call(hh=other._h) == L.SFE_EINVAL and k.value == 0
    assert lib.sfe_dsp_burst_set_gate(other._h, 0.5) == L.SFE_EINVAL and lib.sfe_dsp_burst_set_input_format(other._h, L.FMT_U8) == L.SFE_EINVAL
    assert lib.sfe_dsp_burst_destroy(other._h) == L.SFE_OK
    other.reset()                                                    # still alive
    other.close()
    assert lib.sfe_dsp_burst_set_gate(h._h, np.nan) == L.SFE_EINVAL and lib.sfe_dsp_last_error().startswith(b"burst: ")
    assert lib.sfe_dsp_burst_set_input_format(h._h, 7) == L.SFE_EINVAL
    with pytest.raises(AttributeError):
        h.reset()
    api.sync()
    for d in (d_out, d_rec, d_st):
        assert np.array_equal(_bits(d.to_numpy()), _bits(sentinel))
    # the next good call is a fresh handle's, and set_gate is taken from the next call on
    assert call() == L.SFE_OK and k.value == nb
    want = api.Burst(preamble_of(sps, Lp, 7), sps, N, lag, n_streams=S).demodulate(x, idx=np.zeros((S, nb)), gate=np.ones((S, nb)), start_base=sps,
                                                                              start_step=2)
    assert not want[2].any()
    assert np.array_equal(_bits(d_out.to_numpy(S * nb * N * 2)), _bits(want[0]).ravel())
    assert np.array_equal(_bits(d_rec.to_numpy(S * nb * 8)), _bits(want[1]).ravel())
    assert np.array_equal(d_st.to_numpy(S * nb).view(np.int32), want[2].ravel())
    h.set_gate(1.5)
    assert call() == L.SFE_OK and d_st.to_numpy(S * nb).view(np.int32).tolist() == [2] * (S * nb)
    h.close()
    for d in (d_in, d_idx, d_gate, d_out, d_rec, d_st):
        d.free()
