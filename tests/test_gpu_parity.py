"""Parity of the HIP path (through the C ABI, libsfe_dsp.so) against the CPU oracle and the
committed golden vectors.  Needs a real MI355X: run with `-m gpu`.

Bars: bit-exact for resample/decimate in exact mode (integer and general rates);
rel-RMS <= 1e-5 (BASELINE.json north_star) for the FFT FIR and the fused-multiply-add modes.
"""
import numpy as np
import pytest

import stream_checks as sc
from simplefe_amd import synth

pytestmark = pytest.mark.gpu

TOL = 1e-5   # north_star: "within 1e-5 RMS of the fftw3 CPU reference"


@pytest.fixture(scope="module")
def api():
    from simplefe_amd import api as a
    assert a.device_count() >= 1, "no GPU visible"
    return a


@pytest.fixture(scope="module")
def L():
    from simplefe_amd import lib
    return lib


@pytest.fixture(autouse=True)
def _guards():
    """every buffer of a test (stream_checks.Guarded): guards still poison, inputs still what was uploaded"""
    yield
    sc.check_guarded()


def oracle_fir_cf32(orc, taps, x_il, fft_len=4096):
    """A cf32 stream through real taps = two real blkconv passes."""
    yr = orc.Blkconv(taps, fft_len).stream(x_il[0::2])
    yi = orc.Blkconv(taps, fft_len).stream(x_il[1::2])
    y = np.empty_like(x_il)
    y[0::2], y[1::2] = yr, yi
    return y


def oracle_fir_cf32_ctaps(orc, tr, ti, x_il, fft_len=4096):
    """Complex taps: yr = hr*xr - hi*xi, yi = hr*xi + hi*xr -- four real passes."""
    xr, xi = x_il[0::2], x_il[1::2]
    f = lambda t, x: orc.Blkconv(t, fft_len).stream(x)
    y = np.empty_like(x_il)
    y[0::2] = f(tr, xr) - f(ti, xi)
    y[1::2] = f(tr, xi) + f(ti, xr)
    return y


# --------------------------------------------------------------------------- plumbing
def test_synth_fill_matches_host_twin(api):
    for n, first, ch in ((4096, 0, 0), (1001, 12345, 3), (7, 2 ** 33 + 5, 1)):
        d = sc.device_array(api, n + 8)
        d.fill_synth(synth.SEED, channel=ch, first=first, n_floats=n)
        assert np.array_equal(d.to_numpy(n), synth.synth_f32(n, synth.SEED, ch, first))


# ------------------------------------------------------------------------------- FIR
@pytest.mark.parametrize("n", [50000, 3840, 3841, 1, 255, 4096 * 3])
def test_fir_fft_cf32_256taps_vs_oracle(api, L, orc, n):
    taps = synth.taps_cfg2()
    x = synth.synth_cf32(n)
    y = sc.fir_filter(api, api.Fir(taps, data_complex=True, algo=L.FIR_ALGO_FFT), x)[0]
    ref = oracle_fir_cf32(orc, taps, x)
    assert synth.rel_rms(y, ref) <= TOL
    # and against the mathematical definition in float64
    r64 = np.convolve(x[0::2].astype(np.float64), taps.astype(np.float64))[:n]
    assert synth.rel_rms(y[0::2], r64) <= TOL


def test_fir_fft_complex_taps(api, L, orc):
    tr, ti = synth.complex_taps(256, 0.2)
    x = synth.synth_cf32(30000)
    y = sc.fir_filter(api, api.Fir(tr + 1j * ti, data_complex=True, algo=L.FIR_ALGO_FFT), x)[0]
    ref = oracle_fir_cf32_ctaps(orc, tr, ti, x)
    assert synth.rel_rms(y, ref) <= TOL


@pytest.mark.parametrize("n_taps", [1, 2, 63, 257, 258, 1000, 3841])
def test_fir_fft_tap_counts(api, L, n_taps):
    rng = np.random.default_rng(n_taps)
    taps = (rng.standard_normal(n_taps) / np.sqrt(n_taps)).astype(np.float32)
    x = synth.synth_cf32(20000)
    y = sc.fir_filter(api, api.Fir(taps, data_complex=True, algo=L.FIR_ALGO_FFT), x)[0]
    from scipy.signal import fftconvolve
    for c in (0, 1):
        r64 = fftconvolve(x[c::2].astype(np.float64), taps.astype(np.float64))[:20000]
        assert synth.rel_rms(y[c::2], r64) <= TOL, (n_taps, c)


def test_fir_cfg1_real_63taps_2pow20(api, orc):
    """BASELINE cfg1 shape on the GPU path: real float32, 63 taps, 2^20 samples."""
    taps = synth.taps_cfg1()
    x = synth.synth_f32(1 << 20)
    y = sc.fir_filter(api, api.Fir(taps, data_complex=False), x)[0]
    ref = orc.Blkconv(taps, 1024).stream(x)
    assert synth.rel_rms(y, ref) <= TOL


def test_fir_direct_matches_fft_and_oracle(api, L, orc):
    taps = synth.taps_cfg2()
    x = synth.synth_cf32(40000)
    yd = sc.fir_filter(api, api.Fir(taps, data_complex=True, algo=L.FIR_ALGO_DIRECT), x)[0]
    yf = sc.fir_filter(api, api.Fir(taps, data_complex=True, algo=L.FIR_ALGO_FFT), x)[0]
    ref = oracle_fir_cf32(orc, taps, x)
    assert synth.rel_rms(yd, ref) <= TOL
    assert synth.rel_rms(yf, yd) <= TOL


@pytest.mark.parametrize("algo", ["FIR_ALGO_FFT", "FIR_ALGO_DIRECT"])
def test_fir_state_carried_across_calls(api, L, algo):
    """Chunked calls == one call (the overlap state of blkconv.cxx:105-109)."""
    taps = synth.taps_cfg2()
    n = 30000
    x = synth.synth_cf32(n)
    whole = sc.fir_filter(api, api.Fir(taps, data_complex=True, algo=getattr(L, algo)), x)[0]
    f = api.Fir(taps, data_complex=True, algo=getattr(L, algo))
    parts = []
    cuts = [0, 100, 101, 4000, 4100, 12345, n]
    for a, b in zip(cuts[:-1], cuts[1:]):
        parts.append(sc.fir_filter(api, f, x[2 * a:2 * b])[0])
    assert synth.rel_rms(np.concatenate(parts), whole) <= 2e-6
    f.reset()
    assert synth.rel_rms(sc.fir_filter(api, f, x)[0], whole) == 0.0


def test_fir_multichannel_strided(api, L):
    taps = synth.taps_cfg2()
    nch, n, stride = 5, 9000, 9100
    x = np.zeros((nch, 2 * stride), dtype=np.float32)
    for c in range(nch):
        x[c, : 2 * n] = synth.synth_cf32(n, ch=c)
    d_in = sc.from_numpy(api, x)
    d_out = sc.device_array(api, nch * 2 * stride)
    d_out.zero()
    f = api.Fir(taps, data_complex=True, n_channels=nch, algo=L.FIR_ALGO_FFT)
    f.process_stream(d_in, d_out, n, in_stride=stride, out_stride=stride)
    y = d_out.to_numpy().reshape(nch, 2 * stride)
    single = api.Fir(taps, data_complex=True, algo=L.FIR_ALGO_FFT)
    for c in range(nch):
        single.reset()
        assert np.array_equal(y[c, : 2 * n], sc.fir_filter(api, single, x[c, : 2 * n])[0]), c
        assert not y[c, 2 * n:].any()       # padding untouched


@pytest.mark.parametrize("n_taps,ctaps", [(256, False), (63, True), (1000, False)])
def test_fir_per_channel_taps(api, L, orc, n_taps, ctaps):
    """sfe_dsp_fir_create_per_channel: every channel its own filter (what several reference objects with
    different taps are), one launch for all of them, state carried across two calls.  Each channel against
    a single-channel handle with that channel's taps (same transform arithmetic) and against the oracle."""
    rng = np.random.default_rng(n_taps)
    nch, n, stride = 5, 20000, 20480
    taps = rng.standard_normal((nch, n_taps)).astype(np.float32) / np.sqrt(n_taps)
    if ctaps:
        taps = (taps + 1j * rng.standard_normal((nch, n_taps)).astype(np.float32) / np.sqrt(n_taps)).astype(np.complex64)
    x = np.zeros((nch, 2 * stride), dtype=np.float32)
    for c in range(nch):
        x[c, : 2 * n] = synth.synth_cf32(n, ch=20 + c)
    d_in = sc.from_numpy(api, x)
    d_out = sc.device_array(api, nch * 2 * stride)
    f = api.Fir(taps, per_channel=True)
    cut = 7777
    f.process_stream(d_in, d_out, cut, in_stride=stride, out_stride=stride)
    y1 = d_out.to_numpy(keep=True).reshape(nch, 2 * stride)[:, : 2 * cut].copy()
    f.process_stream(d_in.ptr + 8 * cut, d_out.ptr + 8 * cut, n - cut, in_stride=stride, out_stride=stride)
    y = d_out.to_numpy().reshape(nch, 2 * stride)
    assert np.array_equal(y[:, : 2 * cut], y1)
    for c in range(nch):
        one = sc.fir_filter(api, api.Fir(taps[c], data_complex=True, algo=L.FIR_ALGO_FFT), x[c, : 2 * n])[0]
        assert synth.rel_rms(y[c, : 2 * n], one) <= 1e-6, c
        xr, xi = x[c, 0:2 * n:2], x[c, 1:2 * n:2]
        if ctaps:
            hr, hi = np.real(taps[c]).astype(np.float32), np.imag(taps[c]).astype(np.float32)
            rr, ii = orc.Blkconv(hr, 4096 if n_taps <= 2048 else 8192).stream(xr), orc.Blkconv(hi, 4096).stream(xi)
            ri, ir = orc.Blkconv(hr, 4096).stream(xi), orc.Blkconv(hi, 4096).stream(xr)
            ref_re, ref_im = rr - ii, ri + ir
        else:
            ref_re = orc.Blkconv(taps[c], 4096).stream(xr)
            ref_im = orc.Blkconv(taps[c], 4096).stream(xi)
        assert synth.rel_rms(y[c, 0:2 * n:2], ref_re) <= TOL and synth.rel_rms(y[c, 1:2 * n:2], ref_im) <= TOL, c


def test_blkconv_class_known_answer(api, g1):
    """libdsp/test/test_blkconv.cxx:5-33 through the drop-in class."""
    c = api.blkconv(g1["taps"], int(g1["fft_len"]))
    assert c.get_blksize() == int(g1["blksize"])
    buf = c.get_process_buf()
    buf[: c.get_blksize()] = g1["in1"]
    c.process()
    assert np.allclose(buf[: c.get_blksize()], g1["out1"], atol=float(g1["print_tol"]))
    buf[: c.get_blksize()] = g1["in2"]
    c.process()
    assert np.allclose(buf[: c.get_blksize()], g1["out2"], atol=float(g1["print_tol"]))


def test_blkconv_class_pulse_shaping(api, orc, g1):
    """bpsk.cxx:122-164 calling pattern: 111 taps, fft 2048, block by block."""
    c = api.blkconv(g1["g2_taps"], int(g1["g2_fft_len"]))
    blk = c.get_blksize()
    buf = c.get_process_buf()
    x = g1["g2_x"]
    y = np.empty_like(x)
    for off in range(0, len(x), blk):
        buf[:blk] = x[off:off + blk]
        c.process()
        y[off:off + blk] = buf[:blk]
    assert synth.rel_rms(y, g1["g2_y64"]) <= TOL
    assert synth.rel_rms(y, orc.Blkconv(g1["g2_taps"], int(g1["g2_fft_len"])).stream(x)) <= TOL


# ------------------------------------------------------------- resample / decimate
RATES = ("1p77", "5o3", "8", "2p5")


def _drive(obj, x, B, out_len, rate):
    ys, ns = [], []
    for off in range(0, len(x), B):
        n, o = obj.process(x[off:off + B], out_len, rate)
        ys.append(o[:n])
        ns.append(n)
    return np.concatenate(ys), ns


G7_SEEN = {}


@pytest.mark.parametrize("name", ["kat", "bpsk", "cfg1", "cfg2", "rrc551"])
def test_blkconv_class_vs_reference_on_its_own_fftw(api, orc, g7, name):
    """THE PIN AT THE FFTW BOUNDARY.  g7 holds outputs of the reference itself
    -- libdsp/blkconv.cxx:34-110 calling its own vendored FFTW 3.3.5 binary, run in the authoring
    container (oracle/pe/, tests/golden/make_golden_fftw.py).  The drop-in class is driven the way
    the reference's callers drive theirs (write [0, blk) of get_process_buf(), process(), read it
    back), and the device-resident stream call is fed the same samples in one piece.
    Tolerance: rel-RMS <= 1e-5 (north_star); observed figures are printed and bounded at 5e-7."""
    taps, fft_len, x, want = g7[f"{name}_taps"], int(g7[f"{name}_fft_len"]), g7[f"{name}_x"], g7[f"{name}_y"]
    c = api.blkconv(taps, fft_len)
    blk = c.get_blksize()
    buf = c.get_process_buf()
    assert blk == fft_len + 1 - len(taps)
    got = np.empty_like(x)
    for off in range(0, len(x), blk):
        buf[:blk] = x[off: off + blk]
        c.process()
        got[off: off + blk] = buf[:blk]
    e_class = synth.rel_rms(got, want)
    bulk = sc.fir_filter(api, api.Fir(taps, data_complex=False), x).reshape(-1)
    e_bulk = synth.rel_rms(bulk, want)
    G7_SEEN[name] = (e_class, e_bulk)
    print(f"g7 {name}: class {e_class:.3e}  stream {e_bulk:.3e}  max abs {np.abs(got - want).max():.3e}")
    assert e_class <= TOL and e_bulk <= TOL
    assert e_class < 5e-7 and e_bulk < 5e-7
    assert np.abs(got - want).max() < 2e-6 * max(1.0, float(np.abs(want).max()))


@pytest.mark.parametrize("name", ["kat", "bpsk", "cfg1", "cfg2"])
def test_blkconv_class_vs_reference_class(api, orc, g6, name):
    """The drop-in blkconv class against the reference's own (blkconv.cxx on libhipfftw): the
    committed outputs (g6), and the compiled reference run live here beside it when the prebuilt
    oracle/_ref/libsferef_blkconv.so travelled with the snapshot.  Same calls as the
    reference's callers: write [0, blk) of get_process_buf(), process(), read it back."""
    taps, fft_len, x, want = g6[f"{name}_taps"], int(g6[f"{name}_fft_len"]), g6[f"{name}_x"], g6[f"{name}_y"]
    c = api.blkconv(taps, fft_len)
    blk = c.get_blksize()
    buf = c.get_process_buf()
    assert blk == fft_len + 1 - len(taps)
    got = np.empty_like(x)
    for off in range(0, len(x), blk):
        buf[:blk] = x[off: off + blk]
        c.process()
        got[off: off + blk] = buf[:blk]
    assert synth.rel_rms(got, want) <= TOL
    assert synth.rel_rms(got, want) < 1e-6            # what is actually observed: ~3e-7
    if orc.ref_blkconv_lib() is not None:
        live = orc.RefBlkconv(taps, fft_len).stream(x)
        assert synth.rel_rms(live, want) < 1e-6       # hipFFT plans may differ between boxes: rounding only
        assert synth.rel_rms(got, live) < 1e-6


@pytest.mark.parametrize("cls", ["resample", "decimate"])
@pytest.mark.parametrize("tag", RATES + ("0p77",))
def test_rs_class_reference_vector_bit_exact(api, g4, cls, tag):
    """The reference's own driver (test_decimate.py:22-25 / test_resample.py:22-25) against
    outputs of the compiled reference: same n_out per call, same bits."""
    if cls == "decimate" and tag == "0p77":
        pytest.skip("decimate rejects rate < 1 (decimate.cxx:75)")
    B = int(g4["B"])
    obj = getattr(api, cls)(g4["taps"], int(g4["U"]), B)
    y, ns = _drive(obj, g4["x"], B, 4 * B, float(g4[f"rate_{tag}"]))
    assert ns == g4[f"n_{tag}"].tolist()
    assert np.array_equal(y, g4[f"y_{tag}"])


def _tight_out_lens(orc, cls, g4, U, B, rate, x, slack):
    """Drive the oracle with per-call out_len = the call's natural output count + slack; returns
    (out_len, n_out, outputs) per call.  The natural count comes from a second oracle object kept in
    step (slack >= 1 never ends a call on the buffer test, so both objects stay in the same state)."""
    obj = getattr(orc, cls.capitalize())(g4["taps"], U, B)
    twin = getattr(orc, cls.capitalize())(g4["taps"], U, B)
    calls = []
    for off in range(0, len(x), B):
        seg = x[off:off + B]
        natural, _ = twin.process(seg, 4 * B, rate)
        out_len = natural + slack
        n, y = obj.process(seg, out_len, rate)
        assert n == natural
        calls.append((out_len, n, y[:n].copy()))
    return calls


@pytest.mark.parametrize("cls", ["resample", "decimate"])
@pytest.mark.parametrize("tag", ["1p77", "5o3", "2p5"])
@pytest.mark.parametrize("slack", [1, 2, 3])
def test_rs_class_tight_out_len(api, orc, g4, cls, tag, slack):
    """process() with an output buffer only one to three longer than the call's natural output count:
    at a general rate that can be too tight for the bulk path's planning margin, so the per-output
    schedule runs; at an integer-valued step the bulk path does -- either way the reference's n_out
    and bits, call after call (the oracle is bit-pinned to the compiled reference).  A buffer of
    EXACTLY the natural count ends the reference's loop on the buffer test before it can note a
    left-over output, and its next call indexes the delay line out of range: not a defined case."""
    U, B, rate = int(g4["U"]), int(g4["B"]), float(g4[f"rate_{tag}"])
    x = g4["x"]
    want = _tight_out_lens(orc, cls, g4, U, B, rate, x, slack)
    obj = getattr(api, cls)(g4["taps"], U, B)
    for k, (out_len, nw, yw) in enumerate(want):
        ng, yg = obj.process(x[k * B:(k + 1) * B], out_len, rate)
        assert ng == nw, (k, out_len)
        assert np.array_equal(yg[:ng], yw), (k, out_len)


@pytest.mark.parametrize("cls", ["resample", "decimate"])
@pytest.mark.parametrize("tag", ["1p77", "5o3"])
def test_rs_class_truncating_out_len_first_call(api, orc, g4, cls, tag):
    """A buffer shorter than the natural count ends the call at out_len (resample.cxx:126-128).  One
    call only: after a truncated call the reference's next call indexes its delay line out of range."""
    U, B, rate = int(g4["U"]), int(g4["B"]), float(g4[f"rate_{tag}"])
    seg = g4["x"][:B]
    natural, _ = getattr(orc, cls.capitalize())(g4["taps"], U, B).process(seg, 4 * B, rate)
    out_len = max(int(np.floor(B / rate)), natural - 3)
    nw, yw = getattr(orc, cls.capitalize())(g4["taps"], U, B).process(seg, out_len, rate)
    ng, yg = getattr(api, cls)(g4["taps"], U, B).process(seg, out_len, rate)
    assert ng == nw == out_len
    assert np.array_equal(yg[:ng], yw[:nw])


@pytest.mark.parametrize("name", ["cfg3", "cfg4", "gen", "gen2"])
@pytest.mark.parametrize("B", [4096, 1001])
def test_rs_class_baseline_shapes_bit_exact(api, g5, name, B):
    x = synth.synth_f32(int(g5["n"]), seed=int(g5["seed"]))
    rate = float(g5[f"{name}_rate"])
    obj = api.decimate(g5[f"{name}_taps"], int(g5[f"{name}_U"]), B)
    y, ns = _drive(obj, x, B, int(np.ceil(B / rate)) + 2, rate)
    key = f"{name}_y" if f"{name}_y" in g5.files else f"{name}_y_B{B}"
    assert ns == g5[f"{name}_n_B{B}"].tolist()
    assert np.array_equal(y, g5[key])


@pytest.mark.parametrize("name", ["cfg3", "cfg4"])
@pytest.mark.parametrize("chunk", [None, 4096, 1001, 777])
def test_rs_bulk_integer_step(api, L, g5, name, chunk):
    """Device-resident bulk path, closed-form integer step: exact mode is bit-exact with the
    compiled reference whatever the call chunking; FMA mode within 1e-5."""
    x = synth.synth_f32(int(g5["n"]), seed=int(g5["seed"]))
    rate = float(g5[f"{name}_rate"])
    for exact in (True, False):
        r = api.Rs(g5[f"{name}_taps"], int(g5[f"{name}_U"]), 4096, mode=L.RS_DECIMATE)
        r.set_exact(exact)
        y = sc.resample_array(api, r, x, rate, chunk=chunk)[0]
        gold = g5[f"{name}_y"]
        # the reference's total already leaves a pending "leftover" (resample.cxx:141-145) out: equality
        sc.check_total(len(y), len(gold), len(x), int(g5[f"{name}_U"]), rate, r.get_state())
        if exact:
            assert np.array_equal(y, gold)
        else:
            assert synth.rel_rms(y, gold) <= TOL


@pytest.mark.parametrize("name", ["gen", "gen2"])
def test_rs_bulk_general_rate(api, L, g5, name):
    """Non-integer step: the float32 recurrence is replayed per blksize chunk, so one bulk
    call equals the reference fed in chunks of blksize."""
    x = synth.synth_f32(int(g5["n"]), seed=int(g5["seed"]))
    rate = float(g5[f"{name}_rate"])
    for B in (4096, 1000):
        r = api.Rs(g5[f"{name}_taps"], int(g5[f"{name}_U"]), B, mode=L.RS_RESAMPLE)
        r.set_exact(True)
        y = sc.resample_array(api, r, x, rate)[0]
        assert np.array_equal(y, g5[f"{name}_y_B{B}"])


def test_rs_complex_multichannel(api, L, orc, g5):
    """cf32 through real taps = I and Q as two real passes, 3 channels."""
    taps, U, rate = g5["cfg3_taps"], 3, float(g5["cfg3_rate"])
    n, nch = 20000, 3
    x = np.stack([synth.synth_cf32(n, ch=c) for c in range(nch)])
    r = api.Rs(taps, U, 4096, mode=L.RS_RESAMPLE, data_complex=True, n_channels=nch)
    r.set_exact(True)
    y = sc.resample_array(api, r, x, rate)
    for c in range(nch):
        for part in (0, 1):
            ref, _ = orc.Resample(taps, U, 4096).stream(x[c, part::2], rate)
            got = y[c, part::2]
            sc.check_total(len(got), len(ref), n, U, rate)
            assert np.array_equal(got, ref)


def test_rs_parameter_errors(api, g4, capfd):
    """resample.cxx:91-98 / decimate.cxx:75-87: message on stdout, zero outputs, no exception."""
    r = api.resample(g4["taps"], 4, 128)
    assert r.process(np.zeros(129, np.float32), 512, 1.5)[0] == 0
    assert r.process(np.zeros(128, np.float32), 512, 0.2)[0] == 0
    assert r.process(np.zeros(128, np.float32), 10, 1.5)[0] == 0
    d = api.decimate(g4["taps"], 4, 128)
    assert d.process(np.zeros(128, np.float32), 512, 0.9)[0] == 0
    assert d.process(np.zeros(129, np.float32), 512, 2.0)[0] == 0
    # state untouched by the rejected calls: the next good call behaves like a first call
    n, y = d.process(g4["x"][:128], 512, float(g4["rate_8"]))
    assert n == int(g4["n_8"][0]) and np.array_equal(y[:n], g4["y_8"][:n])


def test_rs_bulk_out_cap_too_small(api, L, g5):
    r = api.Rs(g5["cfg4_taps"], 1, 4096, mode=L.RS_DECIMATE)
    d_in = sc.device_array(api, 8000)
    d_out = sc.device_array(api, 16)
    with pytest.raises(api.SfeError) as e:
        r.process_stream(d_in, 8000, d_out, 16, 8.0)
    assert e.value.code == L.SFE_ERANGE


# ------------------------------------------------------------------------ converters
def test_converters_bit_exact(api, L, orc):
    rng = np.random.default_rng(11)
    b = rng.integers(0, 256, size=4099, dtype=np.uint8)
    lib = L.load()
    import ctypes as C
    d_b = sc.device_array(api, 1100)
    api.check(lib.sfe_dsp_memcpy_h2d(d_b.ptr, b.ctypes.data, b.nbytes, None))
    d_f = sc.device_array(api, len(b) + 4)
    api.check(lib.sfe_dsp_rx_u8_to_f32(d_b.ptr, d_f.ptr, len(b), None))
    assert np.array_equal(d_f.to_numpy(len(b)), orc.rx_u8_to_f32(b))
    x = np.concatenate([rng.uniform(-1, 1, 4000), [0.0, 1.0, -1.0, 0.999, -0.999, 0.5, -0.5, 1e-3]]).astype(np.float32)
    d_x = sc.from_numpy(api, x)
    d_o = sc.device_array(api, len(x) * 5 // 16 + 8)
    api.check(lib.sfe_dsp_tx_f32_to_10bit(d_x.ptr, d_o.ptr, len(x), None))
    out = d_o.to_numpy().view(np.uint8)[: len(x) // 4 * 5]
    assert np.array_equal(out, orc.tx_f32_to_10bit(x))
    # group counts of every residue mod 4 (the kernel packs four groups per thread, tail bytewise),
    # a byte-unaligned destination, and floats left over after the last whole group
    for n_floats, off in ((4 * 13, 0), (4 * 14 + 1, 0), (4 * 15 + 3, 1), (4 * 16 + 2, 3), (4 * 1001, 2), (3, 0)):
        d_o.zero()
        api.check(lib.sfe_dsp_tx_f32_to_10bit(d_x.ptr, d_o.ptr + off, n_floats, None))
        raw = d_o.to_numpy().view(np.uint8)
        want = orc.tx_f32_to_10bit(x[:n_floats])
        assert np.array_equal(raw[off: off + len(want)], want) and not raw[off + len(want): off + len(want) + 8].any()


# ------------------------------------------------- matrix-pipe (f32 MFMA) polyphase path
@pytest.mark.parametrize("name,force", [("cfg3", True), ("cfg4", True), ("gen2_int", True)])
@pytest.mark.parametrize("chunk", [None, 5000, 1001])
def test_rs_bulk_mfma_path_cf32(api, L, orc, g5, monkeypatch, name, force, chunk):
    """The opt-in f32-MFMA form of the bulk path (sfe_dsp_rs_set_algo MFMA) on cf32 data: 5/3 resampler
    (78 % dense tap matrix), 7/3 (odd step), and decimate/8, whose plan does not fit and must fall
    back to the VALU kernel silently.  Versus the oracle, I and Q as
    two real passes; chunked calls exercise every carried pos0."""
    if name == "gen2_int":
        taps, U, rate = g5["cfg3_taps"], 3, 7.0 / 3.0
    else:
        taps, U, rate = g5[f"{name}_taps"], int(g5[f"{name}_U"]), float(g5[f"{name}_rate"])
    n, nch = 40000, 2
    x = np.stack([synth.synth_cf32(n, ch=c) for c in range(nch)])
    r = api.Rs(taps, U, 4096, mode=L.RS_RESAMPLE, data_complex=True, n_channels=nch,
               algo=L.RS_ALGO_MFMA if force else L.RS_ALGO_AUTO)
    y = sc.resample_array(api, r, x, rate, chunk=chunk)
    for c in range(nch):
        for part in (0, 1):
            ref, _ = orc.Resample(taps, U, 4096).stream(x[c, part::2], rate)
            got = y[c, part::2]
            sc.check_total(len(got), len(ref), n, U, rate)
            assert synth.rel_rms(got, ref) <= TOL, (c, part)


# ------------------------------------------------- transform-domain polyphase path (poly_fft.hip)
@pytest.mark.parametrize("U,S,n_taps,n,nch,chunk", [
    (3, 5, 381, 100000, 1, None), (3, 5, 381, 250001, 2, 65536), (2, 3, 200, 90000, 1, None),
    (2, 5, 301, 90000, 3, 40000), (3, 4, 255, 120000, 1, None), (1, 2, 128, 80000, 1, 30000),
    (1, 3, 200, 80000, 1, None), (1, 4, 256, 80000, 2, None), (1, 5, 333, 80000, 1, 20001),
    (3, 5, 30, 60000, 1, None), (3, 5, 1000, 200000, 1, 70000), (6, 10, 762, 100000, 1, None),
    (3, 5, 381, 8000, 1, None), (3, 5, 1420, 50000, 1, None), (3, 5, 2860, 60000, 1, 25000),
    (1, 6, 400, 90000, 1, None), (1, 7, 500, 100000, 2, 50001), (1, 8, 600, 120000, 1, None),
    (2, 7, 450, 100000, 1, 33000), (4, 5, 700, 90000, 1, None), (3, 5, 381, 30000, 19, None)])
def test_rs_bulk_fft_path_cf32(api, L, orc, monkeypatch, U, S, n_taps, n, nch, chunk):
    """Every instantiated (SP, UP) of the 256-point transform-domain kernel, forced on
    (sfe_dsp_rs_set_algo FFT), against the oracle with I and Q as two real passes: ragged ends, chunked calls
    (carried history and pos0), channel strides, a filter too short to need it, one whose overlap
    (Li = 192 low-rate taps of every 256 points) is the longest it accepts, and a stream of few segments."""
    rng = np.random.default_rng(U * 100 + S)
    taps = (rng.standard_normal(n_taps) / np.sqrt(n_taps)).astype(np.float32)
    x = np.stack([synth.synth_cf32(n, ch=10 + c) for c in range(nch)])
    r = api.Rs(taps, U, 4096, mode=L.RS_RESAMPLE, data_complex=True, n_channels=nch, algo=L.RS_ALGO_FFT)
    y = sc.resample_array(api, r, x, float(np.float32(S) / np.float32(U)), chunk=chunk)
    for c in range(nch):
        for part in (0, 1):
            ref, _ = orc.Resample(taps, U, 4096).stream(x[c, part::2], float(np.float32(S) / np.float32(U)))
            got = y[c, part::2]
            sc.check_total(len(got), len(ref), n, U, float(np.float32(S) / np.float32(U)))
            assert synth.rel_rms(got, ref) <= TOL, (c, part)


@pytest.mark.parametrize("chunk", [None, 70000])
def test_rs_fft_path_channels_in_one_launch_equal_one_handle_per_channel(api, L, chunk):
    """Round 3: the transform-domain kernel draws the passes of ALL channels from its work counters
    (channel-major tickets) and writes every channel's next history itself.  Seven channels through
    one handle -- one launch per call -- give, channel for channel and bit for bit, what seven
    single-channel handles give, over chunked calls (carried history and time state per channel)."""
    taps, U, S = synth.taps_cfg3(), 3, 5
    rate = float(np.float32(S) / np.float32(U))
    n, nch = 210007, 7
    x = np.stack([synth.synth_cf32(n, ch=30 + c) for c in range(nch)])
    many = api.Rs(taps, U, 4096, mode=L.RS_RESAMPLE, data_complex=True, n_channels=nch, algo=L.RS_ALGO_FFT)
    y = sc.resample_array(api, many, x, rate, chunk=chunk)
    for c in range(nch):
        one = api.Rs(taps, U, 4096, mode=L.RS_RESAMPLE, data_complex=True, algo=L.RS_ALGO_FFT)
        yc = sc.resample_array(api, one, x[c:c + 1], rate, chunk=chunk)[0]
        assert yc.shape == y[c].shape and np.array_equal(yc, y[c]), c
        one.close()


@pytest.mark.parametrize("U,S,n_taps,n,nch,chunk", [
    (3, 5, 381, 100000, 1, None), (3, 5, 381, 250001, 2, 65536), (2, 3, 200, 90001, 1, None),
    (1, 4, 256, 80000, 2, 30001), (1, 8, 600, 120000, 1, None), (4, 5, 700, 90000, 1, None),
    (3, 5, 381, 7001, 1, None), (3, 5, 381, 5 * 231 * 3, 1, None)])
def test_rs_bulk_fft_path_real_data(api, L, orc, monkeypatch, U, S, n_taps, n, nch, chunk):
    """Real float32 streams through the transform-domain kernel: two consecutive real segments
    ride as the real and imaginary parts of one transform (the sub-filters are real).  Odd and
    even segment counts, streams ending inside the first / second half of a pair, chunked calls."""
    rng = np.random.default_rng(U * 1000 + S)
    taps = (rng.standard_normal(n_taps) / np.sqrt(n_taps)).astype(np.float32)
    x = np.stack([synth.synth_f32(n, ch=20 + c) for c in range(nch)])
    rate = float(np.float32(S) / np.float32(U))
    r = api.Rs(taps, U, 4096, mode=L.RS_RESAMPLE, data_complex=False, n_channels=nch, algo=L.RS_ALGO_FFT)
    y = sc.resample_array(api, r, x, rate, chunk=chunk)
    for c in range(nch):
        ref, _ = orc.Resample(taps, U, 4096).stream(x[c], rate)
        sc.check_total(len(y[c]), len(ref), n, U, rate)
        assert synth.rel_rms(y[c], ref) <= TOL, c


@pytest.mark.parametrize("U,S,n_taps", [(1, 4, 256), (1, 5, 333), (2, 6, 400), (1, 8, 640)])
def test_rs_bulk_fft_path_decimate_mode(api, L, orc, monkeypatch, U, S, n_taps):
    """The decimate class's bulk path (mode DECIMATE: its own tap folding, decimate.cxx:37-66)
    takes the transform-domain kernel for long filters by default; against the oracle's Decimate."""
    rng = np.random.default_rng(S * 10 + U)
    taps = (rng.standard_normal(n_taps) / np.sqrt(n_taps)).astype(np.float32)
    n = 150001
    x = synth.synth_cf32(n, ch=7)[None, :]
    rate = float(np.float32(S) / np.float32(U))
    r = api.Rs(taps, U, 4096, mode=L.RS_DECIMATE, data_complex=True)
    y = sc.resample_array(api, r, x, rate, chunk=70000)[0]
    r2 = api.Rs(taps, U, 4096, mode=L.RS_DECIMATE, data_complex=True)
    r2.set_exact(True)
    ye = sc.resample_array(api, r2, x, rate, chunk=70000)[0]
    assert y.shape == ye.shape and not np.array_equal(y, ye)      # a different kernel served the default
    for part in (0, 1):
        ref, _ = orc.Decimate(taps, U, 4096).stream(x[0, part::2], rate)
        got = y[part::2]
        sc.check_total(len(got), len(ref), n, U, rate)
        assert synth.rel_rms(got, ref) <= TOL
        assert np.array_equal(ye[part::2], ref[: len(got)])       # exact mode: the reference's bits


def test_rs_fft_path_is_the_default_for_long_filters(api, L, g5, monkeypatch):
    """cfg3 (5/3, 381 taps) takes the transform-domain kernel by default and the direct kernel
    with sfe_dsp_rs_set_algo(DIRECT) or in exact mode; the two agree to float32 rounding and the exact one is
    bit-identical with the oracle's law (checked elsewhere), so the default is within tolerance."""
    taps, U, rate = g5["cfg3_taps"], 3, float(g5["cfg3_rate"])
    x = synth.synth_cf32(300000, ch=3)[None, :]
    ys = []
    for algo, exact in ((L.RS_ALGO_AUTO, False), (L.RS_ALGO_DIRECT, False), (L.RS_ALGO_AUTO, True)):
        r = api.Rs(taps, U, 4096, mode=L.RS_RESAMPLE, data_complex=True, algo=algo)
        r.set_exact(exact)
        ys.append(sc.resample_array(api, r, x, rate)[0])
        r.close()
    assert ys[0].shape == ys[1].shape == ys[2].shape
    assert not np.array_equal(ys[0], ys[1])            # different kernels, different rounding
    assert synth.rel_rms(ys[0], ys[2]) <= TOL and synth.rel_rms(ys[1], ys[2]) <= TOL


# ------------------------------------------------ fused receive converter (u8 wire format, N2)
def _u8_stream(n_bytes, seed):
    return np.random.default_rng(seed).integers(0, 256, size=n_bytes, dtype=np.uint8)


def test_fir_u8_input_fused(api, L, orc):
    """FIR reading (I,Q) byte pairs directly == FIR of the converted floats, bit for bit (the
    conversion (b-128)/127 is exact, gr-simplefe source_c_impl.cc:121-132), across chunked calls;
    and within tolerance of the oracle chain converter -> blkconv."""
    taps = synth.taps_cfg2()
    n = 50000
    b = _u8_stream(2 * n, 1)
    xf = orc.rx_u8_to_cf32(b)
    f_ref = api.Fir(taps, data_complex=True, algo=L.FIR_ALGO_FFT)
    want = sc.fir_filter(api, f_ref, xf)[0]
    f = api.Fir(taps, data_complex=True, algo=L.FIR_ALGO_FFT)
    f.set_input_format(L.FMT_U8)
    got = []
    for a, e in ((0, 7777), (7777, 7778), (7778, 30001), (30001, n)):
        d_in = sc.from_bytes(api, b[2 * a:2 * e])
        d_out = sc.device_array(api, 2 * (e - a))
        f.process_stream(d_in, d_out, e - a)
        got.append(d_out.to_numpy())
    got = np.concatenate(got)
    assert synth.rel_rms(got, want) <= 2e-6           # chunk seams move transform boundaries
    one = api.Fir(taps, data_complex=True, algo=L.FIR_ALGO_FFT)
    one.set_input_format(L.FMT_U8)
    d_in = sc.from_bytes(api, b)
    d_out = sc.device_array(api, 2 * n)
    one.process_stream(d_in, d_out, n)
    assert np.array_equal(d_out.to_numpy(), want)     # same kernel arithmetic, same bits
    ref = oracle_fir_cf32(orc, taps, xf)
    assert synth.rel_rms(got, ref) <= TOL


@pytest.mark.parametrize("n", [100000, 7681, 30000 + 5])
@pytest.mark.parametrize("byte_offset", [0, 3])
def test_fir_u8_input_fused_real_stream(api, L, orc, n, byte_offset):
    """Real u8 stream (source_f wire format, source_f_impl.cc:120-129) through the FIR: two real
    segments per transform, bytes requested as 16-byte lanes when the stream is 16-byte aligned
    and bytewise otherwise -- either way the same bits as filtering the converted floats."""
    taps = synth.taps_cfg2()
    b = _u8_stream(n + 16, 9)
    xf = orc.rx_u8_to_f32(b[byte_offset: byte_offset + n])
    want = sc.fir_filter(api, api.Fir(taps, data_complex=False, algo=L.FIR_ALGO_FFT), xf)[0]
    f = api.Fir(taps, data_complex=False, algo=L.FIR_ALGO_FFT)
    f.set_input_format(L.FMT_U8)
    d_in = sc.from_bytes(api, b)
    d_out = sc.device_array(api, n)
    f.process_stream(d_in.ptr + byte_offset, d_out, n)
    got = d_out.to_numpy()
    assert np.array_equal(got, want)
    ref = orc.Blkconv(taps, 4096).stream(xf)
    assert synth.rel_rms(got, ref) <= TOL


@pytest.mark.parametrize("byte_offset", [0, 2, 6, 16])
def test_u8_input_any_alignment_two_channels(api, L, orc, byte_offset):
    """u8 streams that do not start on a 16-byte boundary (the wide-lane request needs one) and
    whose second channel sits at an odd stride take the 2-byte path: same bits as the float path,
    FIR and transform-domain resampler alike."""
    n, nch, stride = 40000, 2, 40000 + 3
    b = _u8_stream(2 * (stride * nch + 16), 5)
    xf = np.stack([orc.rx_u8_to_cf32(b[byte_offset + 2 * stride * c: byte_offset + 2 * stride * c + 2 * n]) for c in range(nch)])
    d_all = sc.from_bytes(api, b)
    for kind in ("fir", "rs"):
        if kind == "fir":
            taps = synth.taps_cfg2()
            want = sc.fir_filter(api, api.Fir(taps, data_complex=True, n_channels=nch, algo=L.FIR_ALGO_FFT), xf)
            f = api.Fir(taps, data_complex=True, n_channels=nch, algo=L.FIR_ALGO_FFT)
            f.set_input_format(L.FMT_U8)
            d_out = sc.device_array(api, nch * 2 * n)
            f.process_stream(d_all.ptr + byte_offset, d_out, n, in_stride=stride, out_stride=n)
            got = d_out.to_numpy().reshape(nch, 2 * n)
        else:
            taps, U, rate = synth.taps_cfg3(), 3, 5.0 / 3.0
            want = sc.resample_array(api, api.Rs(taps, U, 4096, mode=L.RS_RESAMPLE, data_complex=True, n_channels=nch), xf, rate)
            r = api.Rs(taps, U, 4096, mode=L.RS_RESAMPLE, data_complex=True, n_channels=nch)
            r.set_input_format(L.FMT_U8)
            cap = want.shape[1] // 2 + 8
            d_out = sc.device_array(api, nch * 2 * cap)
            k = r.process_stream(d_all.ptr + byte_offset, n, d_out, cap, rate, in_stride=stride, out_stride=cap)
            got = d_out.to_numpy().reshape(nch, 2 * cap)[:, : 2 * k]
        assert got.shape == want.shape and np.array_equal(got, want), (kind, byte_offset)


@pytest.mark.parametrize("name,cplx", [("cfg4", True), ("cfg4", False), ("cfg3", True)])
@pytest.mark.parametrize("chunk", [None, 4099, 1001])
def test_rs_u8_input_fused(api, L, orc, g5, name, cplx, chunk):
    """decimate/8 and resample 5/3 reading u8 samples directly: bit-identical to the float path
    fed the converted samples in the same calls (fused numerics; long calls of the 5/3 shape take
    the transform-domain kernel, short ones the direct kernel -- odd chunks exercise its 8-byte
    alignment fix-up), and within tolerance of converter -> oracle."""
    taps, U, rate = g5[f"{name}_taps"], int(g5[f"{name}_U"]), float(g5[f"{name}_rate"])
    n = 30000
    w = 2 if cplx else 1
    b = _u8_stream(w * n, 2)
    xf = orc.rx_u8_to_f32(b)
    chunk = chunk or n
    # same chunking for the float path: which kernel serves a call depends on its length
    ref_gpu = sc.resample_array(api, api.Rs(taps, U, 4096, mode=L.RS_RESAMPLE, data_complex=cplx), xf, rate, chunk=chunk)[0]
    r = api.Rs(taps, U, 4096, mode=L.RS_RESAMPLE, data_complex=cplx)
    r.set_input_format(L.FMT_U8)
    outs = []
    for off in range(0, n, chunk):
        m = min(chunk, n - off)
        d_in = sc.from_bytes(api, b[w * off:w * (off + m)])
        cap = int(m / rate) + 8
        d_out = sc.device_array(api, w * cap)
        k = r.process_stream(d_in, m, d_out, cap, rate)
        outs.append(d_out.to_numpy(w * k))
    got = np.concatenate(outs)
    sc.check_total(len(got) // w, len(ref_gpu) // w, n, U, rate, r.get_state())
    assert np.array_equal(got, ref_gpu)
    for part in range(w):
        ref, _ = orc.Resample(taps, U, 4096).stream(xf[part::w], rate)
        sc.check_total(len(got) // w, len(ref), n, U, rate)
        assert synth.rel_rms(got[part::w], ref) <= TOL


# ------------------------------------------- integer-step shapes outside the compiled (SP, UP) tables
# (x2, x3, x4, 2/3, 3/4, 4/3 have had compile-time instantiations of the tiled kernel since the end of round 4; the others run
# poly_rt_kernel -- both forms are held to the same bar here)
RT_SHAPES = [("x2", 2, 1), ("3/4", 4, 3), ("4/3", 3, 4), ("/6", 1, 6), ("/7", 1, 7), ("/16", 1, 16), ("x4", 4, 1),
             ("7/4", 4, 7), ("2/3", 3, 2), ("/13", 1, 13), ("9/8", 8, 9), ("/48", 1, 48),
             ("x3", 3, 1), ("x5", 5, 1), ("x8", 8, 1), ("4/5", 5, 4), ("7/3", 3, 7), ("5/6", 6, 5), ("7/8", 8, 7)]


@pytest.mark.parametrize("name,U,step", RT_SHAPES)
@pytest.mark.parametrize("cplx", [True, False])
def test_rs_shapes_outside_the_compiled_tables(api, L, orc, name, U, step, cplx):
    """VERDICT r3 missing 4: interpolating ratios (UP > SP: what `resample` takes and `decimate` refuses,
    libdsp/resample.cxx:91 / decimate.cxx:75-78) and decimations no compile-time (SP, UP) pair covers run the
    runtime-shape tiled kernel (poly_rt_kernel).  Exact mode is bit-identical to the oracle (itself bit-exact
    with the compiled reference) over ragged chunkings; the fused default is within 1e-5; u8 wire-format input
    is no longer refused for these shapes and equals the float path fed the converted samples bit for bit."""
    rate = float(np.float32(step) / np.float32(U))
    assert float(np.float32(rate) * np.float32(U)) == float(step)
    taps = synth.lowpass_taps(32 * U - (1 if U > 1 else 0), 0.9 * min(1.0 / U, 1.0 / step), gain=float(U))
    w = 2 if cplx else 1
    n = 3 * 4096 * max(1, step // 8) + 777
    x = synth.synth_f32(w * n, ch=31)
    refs = [orc.Resample(taps, U, 4096).stream(x[part::w], rate)[0] for part in range(w)]
    for exact, chunk in ((True, None), (True, 4096), (True, 3 * 4096 + 0), (False, None)):
        r = api.Rs(taps, U, 4096, mode=L.RS_RESAMPLE, data_complex=cplx)
        r.set_exact(exact)
        r.set_algo(L.RS_ALGO_DIRECT)              # the direct kernels are the subject here
        y = sc.resample_array(api, r, x, rate, chunk=chunk)[0]
        for part in range(w):
            got, ref = y[part::w], refs[part]
            sc.check_total(len(got), len(ref), n, U, rate, r.get_state())
            if exact:
                assert np.array_equal(got, ref[: len(got)]), (name, cplx, chunk)
            else:
                assert synth.rel_rms(got, ref[: len(got)]) <= TOL, (name, cplx)
    # u8 wire-format input through the same shape
    b = _u8_stream(w * n, 4)
    xf = orc.rx_u8_to_f32(b)
    rf = api.Rs(taps, U, 4096, mode=L.RS_RESAMPLE, data_complex=cplx)
    rf.set_algo(L.RS_ALGO_DIRECT)
    want = sc.resample_array(api, rf, xf, rate)[0]
    r8 = api.Rs(taps, U, 4096, mode=L.RS_RESAMPLE, data_complex=cplx)
    r8.set_algo(L.RS_ALGO_DIRECT)
    r8.set_input_format(L.FMT_U8)
    d_in = sc.from_bytes(api, b)
    cap = int(n / rate) + 8
    d_out = sc.device_array(api, w * cap)
    k = r8.process_stream(d_in, n, d_out, cap, rate)
    got = d_out.to_numpy(w * k)
    sc.check_total(len(got) // w, len(want) // w, n, U, rate, r8.get_state())
    assert np.array_equal(got, want), name


@pytest.mark.parametrize("name,U,step", [("/3", 1, 3), ("/5", 1, 5), ("/7", 1, 7), ("/9", 1, 9), ("/15", 1, 15), ("/63", 1, 63), ("5/2", 2, 5), ("7/4", 4, 7),
                                         ("9/4", 4, 9), ("9/2", 2, 9), ("7/3", 3, 7), ("9/5", 5, 9), ("13/6", 6, 13), ("9/7", 7, 9), ("11/8", 8, 11),
                                         ("/6", 1, 6), ("/10", 1, 10), ("/12", 1, 12), ("/16", 1, 16), ("/24", 1, 24), ("/48", 1, 48), ("/64", 1, 64),
                                         ("6/5", 5, 6), ("10/3", 3, 10), ("12/5", 5, 12), ("14/4", 4, 14),
                                         ("4/5", 5, 4), ("5/6", 6, 5), ("7/8", 8, 7), ("9/8", 8, 9), ("2/5", 5, 2), ("3/5", 5, 3), ("3/7", 7, 3), ("3/8", 8, 3), ("2/7", 7, 2),
                                         ("x2", 2, 1), ("x3", 3, 1), ("x4", 4, 1), ("x5", 5, 1), ("x8", 8, 1)])
@pytest.mark.parametrize("cplx", [True, False])
def test_rt_shapes_fetched_by_lds_dma_and_read_in_place(api, L, orc, name, U, step, cplx):
    """Round 5 (poly_rt_dma.hip): float32 streams -- complex, and real (libdsp's native type) -- at an input step SP >= 2 with UP = 1 ... 8
    outputs per SP inputs (odd SP: single-sample reads at a conflict-free stride; even SP: 2 or 4 taps per aligned wide read; UP >= 3:
    outputs through the waves' LDS regions), fused arithmetic, take the runtime-shape kernel whose tile lands in the LDS contiguously
    by LDS-DMA and is read in place.  Same law, same accumulation order as poly_rt_kernel: held to the same bar -- within 1e-5 of the
    oracle (libdsp/decimate.cxx:132-140 through orc.Resample), equal to the exact kernel's length, and BIT-IDENTICAL to the
    runtime-shape kernel it replaces, which still serves (a) a stream whose first sample is not on a 16-byte boundary and (b)
    channels at a stride that is not a multiple of 16 bytes -- so the same samples through those two calls must give the same bits.
    Lengths that end inside a tile, two calls with carried state, three channels."""
    rate = float(np.float32(step) / np.float32(U))
    taps = synth.lowpass_taps(32 * U - (1 if U > 1 else 0), 0.9 * min(1.0 / U, 1.0 / step), gain=float(U))
    w = 2 if cplx else 1
    n, nch = 5 * 4096 * max(1, step // 4) + 1235, 3
    x = np.stack([synth.synth_f32(w * n, ch=70 + c) for c in range(nch)])
    refs = [[orc.Resample(taps, U, 4096).stream(np.ascontiguousarray(x[c, part::w]), rate)[0] for part in range(w)] for c in range(nch)]
    cap = int(n / rate) + 16
    cap += (-cap) % 4                               # channels of the output 16 bytes apart

    def run(offset_floats, stride, out_shift=0):
        """the three channels at `stride` samples apart, the buffer shifted by `offset_floats` floats, the output by `out_shift` floats; two calls"""
        buf = np.zeros(offset_floats + w * stride * nch, np.float32)
        for c in range(nch):
            buf[offset_floats + w * stride * c: offset_floats + w * stride * c + w * n] = x[c]
        d = sc.from_numpy(api, buf)
        d_out = sc.device_array(api, out_shift + w * cap * nch)
        r = api.Rs(taps, U, 4096, mode=L.RS_RESAMPLE, data_complex=cplx, n_channels=nch)
        r.set_algo(L.RS_ALGO_DIRECT)
        cut = (n // 2) // 4096 * 4096
        k1 = r.process_stream(d.ptr + 4 * offset_floats, cut, d_out.ptr + 4 * out_shift, cap, rate, in_stride=stride, out_stride=cap)
        k2 = r.process_stream(d.ptr + 4 * offset_floats + 4 * w * cut, n - cut, d_out.ptr + 4 * (out_shift + w * k1), cap - k1, rate, in_stride=stride, out_stride=cap)
        y = d_out.to_numpy()[out_shift:].reshape(nch, w * cap)[:, : w * (k1 + k2)]
        return k1 + k2, y

    al = (n + 3) // 4 * 4
    k, y = run(0, al)                                # 16-byte aligned channels: the LDS-DMA kernel
    ku, yu = run(w, al + 1)                          # first sample one sample off a 16-byte boundary, an odd stride: poly_rt_kernel
    assert k == ku and np.array_equal(y, yu), name
    ko, yo = run(0, al, out_shift=w)                 # the LDS-DMA kernel storing to an output one sample off a 16-byte boundary (no wide stores)
    assert k == ko and np.array_equal(y, yo), name
    for c in range(nch):
        for part in range(w):
            ref = refs[c][part]
            sc.check_total(k, len(ref), n, U, rate)
            assert synth.rel_rms(y[c, part::w], ref) <= TOL, (name, c, part)


@pytest.mark.parametrize("U", [1, 2, 3, 4, 5, 6, 7, 8])
@pytest.mark.parametrize("arm", [32, 31, 30, 29, 6, 3])
def test_real_interpolators_by_register_window(api, L, orc, U, arm):
    """Round 5 (poly_rt_dma.hip: poly_int4_dma_kernel): a REAL float32 stream interpolated by U (input step 1) -- each lane takes four
    consecutive input positions and reads their samples as whole 16-byte groups into a register window.  Arms of 32, 31, 30 and 29 taps move
    the tile's first sample through all four places of its 16-byte group (one compiled form each) and leave 0 ... 3 taps in front of the
    whole groups of four; arms of 6 and 3 taps: one group, none.  Same law (libdsp/resample.cxx:100-114 at an integer step), same
    accumulation order: within 1e-5 of the oracle and BIT-IDENTICAL to poly_rt1_kernel / poly_tiled_kernel<1, U>, which still serve a
    stream that does not start on a 16-byte boundary.  A length that ends inside a tile, two calls with carried state, three channels."""
    taps = synth.lowpass_taps(arm * U - (1 if U > 1 and arm % 2 == 0 else 0), 0.9 / U, gain=float(U))
    rate = float(np.float32(1.0) / np.float32(U))
    n, nch = 3 * 4096 + 1235, 3
    x = np.stack([synth.synth_f32(n, ch=90 + c) for c in range(nch)])
    refs = [orc.Resample(taps, U, 4096).stream(x[c], rate)[0] for c in range(nch)]
    cap = n * U + 16

    def run(offset_floats, stride, out_shift=0):
        buf = np.zeros(offset_floats + stride * nch, np.float32)
        for c in range(nch):
            buf[offset_floats + stride * c: offset_floats + stride * c + n] = x[c]
        d = sc.from_numpy(api, buf)
        d_out = sc.device_array(api, out_shift + cap * nch)
        r = api.Rs(taps, U, 4096, mode=L.RS_RESAMPLE, data_complex=False, n_channels=nch)
        r.set_algo(L.RS_ALGO_DIRECT)
        cut = 2 * 4096 + 4 * 37
        k1 = r.process_stream(d.ptr + 4 * offset_floats, cut, d_out.ptr + 4 * out_shift, cap, rate, in_stride=stride, out_stride=cap)
        k2 = r.process_stream(d.ptr + 4 * offset_floats + 4 * cut, n - cut, d_out.ptr + 4 * (out_shift + k1), cap - k1, rate, in_stride=stride, out_stride=cap)
        return k1 + k2, d_out.to_numpy()[out_shift:].reshape(nch, cap)[:, : k1 + k2]

    al = (n + 3) // 4 * 4
    k, y = run(0, al)                                # 16-byte aligned channels: the register-window kernel
    ku, yu = run(1, al + 1)                          # one float off, an odd stride: the kernels it replaces
    assert k == ku and np.array_equal(y, yu), (U, arm)
    ko, yo = run(0, al, out_shift=1)                 # the same kernel storing to an output that is NOT on a 16-byte boundary (lane-by-lane stores)
    assert k == ko and np.array_equal(y, yo), (U, arm)
    for c in range(nch):
        sc.check_total(k, len(refs[c]), n, U, rate)
        assert synth.rel_rms(y[c], refs[c]) <= TOL, (U, arm, c)


@pytest.mark.parametrize("U,step", [(1, 2), (1, 3), (1, 4), (1, 5), (2, 3), (2, 5), (3, 2), (3, 4), (3, 5), (4, 3), (4, 5), (5, 2), (5, 3), (5, 4)])
@pytest.mark.parametrize("arm", [32, 31, 30, 29, 6])
def test_real_small_steps_by_register_window(api, L, orc, U, step, arm):
    """Round 5 (poly_rt_dma.hip: poly_int4_dma_kernel<UP, SH, SP>): REAL float32 streams at input steps 2 ... 5 with 1 ... 5 outputs per
    step -- decimate by 2 ... 5, 3/2, 5/3, 2/3, 4/5 ... -- through the register-window kernel (four consecutive m per lane, their samples read
    as whole 16-byte groups), also where a compile-time tiled kernel exists (4/3, 4/5, 5/2 and 5/4 measured slower there, keep their kernels and are
    here as controls).  Arms of 32 / 31 / 30 / 29 / 6 taps: all four places of the
    tile's first sample in its 16-byte group, 0 ... 3 taps in front of the whole groups of four.  Same law (libdsp/decimate.cxx:132-140,
    libdsp/resample.cxx:100-114 at an integer step), same accumulation order: within 1e-5 of the oracle and BIT-IDENTICAL to the kernels
    that still serve a stream off a 16-byte boundary (poly_tiled_kernel where the shape has one, else poly_rt_kernel); an output off a
    16-byte boundary; a length that ends inside a tile, two calls with carried state, three channels."""
    taps = synth.lowpass_taps(arm * U - (1 if U > 1 and arm % 2 == 0 else 0), 0.9 * min(1.0 / U, 1.0 / step), gain=float(U))
    rate = float(np.float32(step) / np.float32(U))
    n, nch = 5 * 4096 + 1235, 3
    x = np.stack([synth.synth_f32(n, ch=110 + c) for c in range(nch)])
    refs = [orc.Resample(taps, U, 4096).stream(x[c], rate)[0] for c in range(nch)]
    cap = n * U // step + 16
    cap += (-cap) % 4

    def run(offset_floats, stride, out_shift=0):
        buf = np.zeros(offset_floats + stride * nch, np.float32)
        for c in range(nch):
            buf[offset_floats + stride * c: offset_floats + stride * c + n] = x[c]
        d = sc.from_numpy(api, buf)
        d_out = sc.device_array(api, out_shift + cap * nch)
        r = api.Rs(taps, U, 4096, mode=L.RS_RESAMPLE, data_complex=False, n_channels=nch)
        r.set_algo(L.RS_ALGO_DIRECT)
        cut = 3 * 4096
        k1 = r.process_stream(d.ptr + 4 * offset_floats, cut, d_out.ptr + 4 * out_shift, cap, rate, in_stride=stride, out_stride=cap)
        k2 = r.process_stream(d.ptr + 4 * offset_floats + 4 * cut, n - cut, d_out.ptr + 4 * (out_shift + k1), cap - k1, rate, in_stride=stride, out_stride=cap)
        return k1 + k2, d_out.to_numpy()[out_shift:].reshape(nch, cap)[:, : k1 + k2]

    al = (n + 3) // 4 * 4
    k, y = run(0, al)                                # 16-byte aligned channels: the register-window kernel
    ku, yu = run(1, al + 1)                          # one float off, an odd stride: the kernels it replaces
    assert k == ku and np.array_equal(y, yu), (U, step, arm)
    ko, yo = run(0, al, out_shift=1)                 # the same kernel, its output off a 16-byte boundary
    assert k == ko and np.array_equal(y, yo), (U, step, arm)
    for c in range(nch):
        sc.check_total(k, len(refs[c]), n, U, rate)
        assert synth.rel_rms(y[c], refs[c]) <= TOL, (U, step, arm, c)


@pytest.mark.parametrize("U,step", [(1, 7), (1, 16), (4, 7), (1, 6), (5, 4), (3, 10), (2, 1), (3, 1), (8, 1), (1, 2), (1, 3), (2, 3), (3, 5), (3, 2)])
@pytest.mark.parametrize("cplx", [True, False])
def test_u8_streams_by_lds_dma(api, L, orc, U, step, cplx):
    """Round 5: the receive wire format (u8 offset binary; a complex sample = two bytes: gr-simplefe/lib/source_c_impl.cc, source_f_impl.cc) into
    the LDS-DMA kernels -- the tile's raw bytes fetched by DMA and converted once, four bytes per step, into the float32 tile the kernels
    read in place.  Three ways to the same bits: (a) u8 channels on 16-byte boundaries (the new path), (b) the same bytes one sample off
    at an odd stride (poly_rt_kernel's u8 form, byte loads sample by sample; the compile-time kernels' where the shape has one), (c) the
    float32 path fed the converted samples.  Two calls with carried state, three channels, a length that ends inside a tile."""
    taps = synth.lowpass_taps(32 * U - (1 if U > 1 else 0), 0.9 * min(1.0 / U, 1.0 / step), gain=float(U))
    rate = float(np.float32(step) / np.float32(U))
    w = 2 if cplx else 1
    n, nch = 5 * 4096 * max(1, step // 4) + 1235, 3
    b = np.stack([_u8_stream(w * n, 40 + c) for c in range(nch)])
    cap = n * U // step + 16
    cap += (-cap) % 4
    cut = (n // 2) // 4096 * 4096

    def run_u8(offset_samples, stride):
        buf = np.zeros(w * (offset_samples + stride * nch), np.uint8)
        for c in range(nch):
            buf[w * (offset_samples + stride * c): w * (offset_samples + stride * c) + w * n] = b[c]
        d = sc.from_bytes(api, buf)
        d_out = sc.device_array(api, w * cap * nch)
        r = api.Rs(taps, U, 4096, mode=L.RS_RESAMPLE, data_complex=cplx, n_channels=nch)
        r.set_algo(L.RS_ALGO_DIRECT)
        r.set_input_format(L.FMT_U8)
        k1 = r.process_stream(d.ptr + w * offset_samples, cut, d_out, cap, rate, in_stride=stride, out_stride=cap)
        k2 = r.process_stream(d.ptr + w * (offset_samples + cut), n - cut, d_out.ptr + 4 * w * k1, cap - k1, rate, in_stride=stride, out_stride=cap)
        return k1 + k2, d_out.to_numpy().reshape(nch, w * cap)[:, : w * (k1 + k2)]

    al = (n + 15) // 16 * 16
    k, y = run_u8(0, al)
    ku, yu = run_u8(1, al + 1)
    assert k == ku and np.array_equal(y, yu), (U, step, cplx)
    xf = np.stack([orc.rx_u8_to_f32(b[c]) for c in range(nch)])
    rf = api.Rs(taps, U, 4096, mode=L.RS_RESAMPLE, data_complex=cplx, n_channels=nch)
    rf.set_algo(L.RS_ALGO_DIRECT)
    d = sc.from_numpy(api, np.ascontiguousarray(np.pad(xf, ((0, 0), (0, w * (al - n))))))
    d_out = sc.device_array(api, w * cap * nch)
    k1 = rf.process_stream(d, cut, d_out, cap, rate, in_stride=al, out_stride=cap)
    k2 = rf.process_stream(d.ptr + 4 * w * cut, n - cut, d_out.ptr + 4 * w * k1, cap - k1, rate, in_stride=al, out_stride=cap)
    yf = d_out.to_numpy().reshape(nch, w * cap)[:, : w * (k1 + k2)]
    assert k1 + k2 == k and np.array_equal(y, yf), (U, step, cplx)


@pytest.mark.parametrize("U,step,n_taps", [(1, 128, 32), (1, 250, 64), (1, 1000, 32), (1, 4000, 16), (3, 128, 96), (1, 100, 128), (2, 129, 300), (1, 117, 32), (5, 512, 40),
                                            (9, 10, 285), (15, 16, 477), (24, 25, 768), (10, 9, 317), (160, 147, 5117), (32, 33, 1024), (64, 66, 2040), (160, 147, 20320)])
@pytest.mark.parametrize("cplx", [True, False])
def test_steps_beyond_the_tiled_kernels(api, L, orc, U, step, n_taps, cplx):
    """Round 5: the reference's decimate / resample take ANY rate >= 1 resp. >= 1 / upsample (libdsp/decimate.cxx:75-78, resample.cxx:91);
    until now the bulk call refused integer steps beyond ~117 ("step too large for the LDS tile").  The generic kernel now holds, where the
    outputs' windows do not overlap (step >= upsample * taps per phase), each output's own samples and nothing between them, and shrinks
    its tile where they do overlap; and ratios with more than eight outputs per period (10/9, 16/15, 25/24, 147/160 ...: the same generic kernel,
    its taps transposed in the LDS so that a wave's lanes -- consecutive outputs, consecutive phases -- read different banks; 20 320 taps in 160
    phases, more than the LDS holds beside a tile, stay in memory: refused until now).  Exact mode: the oracle's bits (itself bit-exact with the compiled reference); default mode: within
    1e-5; two calls with carried state; decimate mode where upsample is 1."""
    rate = float(np.float32(step) / np.float32(U))
    taps = synth.lowpass_taps(n_taps, 0.9 * min(1.0 / U, 1.0 / step), gain=float(U))
    w = 2 if cplx else 1
    n = 24 * 4096
    x = synth.synth_f32(w * n, ch=77)
    refs = [orc.Resample(taps, U, 4096).stream(np.ascontiguousarray(x[part::w]), rate)[0] for part in range(w)]
    for exact in (True, False):
        r = api.Rs(taps, U, 4096, mode=L.RS_DECIMATE if U == 1 else L.RS_RESAMPLE, data_complex=cplx)
        r.set_exact(exact)
        y = sc.resample_array(api, r, x, rate, chunk=10 * 4096)[0]
        for part in range(w):
            got, ref = y[part::w], refs[part]
            sc.check_total(len(got), len(ref), n, U, rate, r.get_state())
            assert len(got) > 0, (U, step, len(ref), len(got))
            if exact:
                assert np.array_equal(got, ref[: len(got)]), (U, step, n_taps, cplx)
            else:
                assert synth.rel_rms(got, ref[: len(got)]) <= TOL, (U, step, n_taps, cplx)


@pytest.mark.parametrize("U,rate,n_taps,B", [(1, 128.0, 32, 4096), (1, 1000.0, 16, 4096), (24, 25.0 / 24.0, 768, 4096), (9, 10.0 / 9.0, 285, 4096),
                                             (1, 2.5, 32, 1000), (3, 1.77, 381, 256), (3, 0.77, 96, 1000), (12, 1.003, 84, 256)])
@pytest.mark.parametrize("cplx", [True, False])
def test_u8_input_is_never_refused(api, L, orc, U, rate, n_taps, B, cplx):
    """Round 5: wire-format (u8) input on shapes that have no fused u8 kernel -- integer steps beyond the tiled kernels' reach, general rates
    the transform-domain kernel does not take (small blksize) -- was REFUSED ("u8 input needs a tiled kernel", "outside what the
    transform-domain kernel takes").  Such a call now converts its bytes once into a scratch buffer of the handle and runs the float32
    path: the result equals, bit for bit and call for call, the float32 path fed the oracle's own conversion of the same bytes
    (gr-simplefe/lib/source_c_impl.cc's (b - 128) / 127); two calls with carried state, two channels."""
    rate = float(np.float32(rate))
    taps = synth.lowpass_taps(n_taps, 0.9 * min(1.0 / U, 1.0 / max(rate * U, 1.0)), gain=float(U))
    w = 2 if cplx else 1
    n, nch = 40 * B, 2
    b = np.stack([_u8_stream(w * n, 60 + c) for c in range(nch)])
    xf = np.stack([orc.rx_u8_to_f32(b[c]) for c in range(nch)])
    cap = int(n / rate) + 4 * (n // B) + 64
    outs = []
    for u8 in (True, False):
        r = api.Rs(taps, U, B, mode=L.RS_RESAMPLE, data_complex=cplx, n_channels=nch)
        if u8:
            r.set_input_format(L.FMT_U8)
            d = sc.from_bytes(api, b)
        else:
            d = sc.from_numpy(api, xf)
        esz = w if u8 else 4 * w                       # bytes per sample of the input
        d_out = sc.device_array(api, w * cap * nch)
        cut = 16 * B
        k1 = r.process_stream(d, cut, d_out, cap, rate, in_stride=n, out_stride=cap)
        k2 = r.process_stream(d.ptr + esz * cut, n - cut, d_out.ptr + 4 * w * k1, cap - k1, rate, in_stride=n, out_stride=cap)
        outs.append((k1, k2, d_out.to_numpy().reshape(nch, w * cap)[:, : w * (k1 + k2)]))
    assert outs[0][:2] == outs[1][:2] and outs[0][0] + outs[0][1] > 0, (U, rate, outs[0][:2], outs[1][:2])
    assert np.array_equal(outs[0][2].view(np.uint32), outs[1][2].view(np.uint32)), (U, rate, n_taps, B, cplx)


@pytest.mark.parametrize("B", [8192, 16384, 65536])
@pytest.mark.parametrize("U,rate,n_taps", [(3, 1.77, 381), (3, 0.77, 96), (1, 2.5, 32), (32, 1.77, 4064), (7, 3.3, 70)])
@pytest.mark.parametrize("cplx", [True, False])
def test_general_rate_calls_larger_than_the_lds(api, L, orc, B, U, rate, n_taps, cplx):
    """Round 5: the direct general-rate kernel stages one reference call -- blksize samples -- per workgroup; a blksize of 8192 complex samples
    or more does not fit the LDS and the bulk call fell through to the host-scheduled path (37 ms for 2^24 samples where blksize 4096 takes
    0.5).  Such a call is now dealt to several workgroups, each with the input span its outputs reach.  Exact mode: the oracle's bits and its
    per-call output counts (libdsp/resample.cxx:100-148 replayed call by call); the fused direct kernel within 1e-5."""
    if (rate < 1.0 and B > 8192) or (B == 65536 and U > 3):
        # 16384 samples x 3 phases at a step of 2.31 (65536 x 7 at 23.1, 65536 x 32 at 56.6): the float32 recurrence drifts by more outputs than the ceil(n_in / rate) + 2 a call may emit,
        # the reference's object is left in its out_len-exhausted state (m_pos < -1) and its NEXT call indexes m_out[][] at
        # negative positions -- undefined behaviour there, a segmentation fault in the oracle's faithful restatement.  Nothing to compare with.
        pytest.skip("the reference's own out_len-exhausted state: its next call reads out of bounds")
    rate = float(np.float32(rate))
    taps = synth.lowpass_taps(n_taps, 0.9 * min(1.0 / U, 1.0 / max(rate * U, 1.0)), gain=float(U))
    w = 2 if cplx else 1
    n = 5 * B + B // 3
    x = synth.synth_f32(w * n, ch=88)
    refs = [orc.Resample(taps, U, B).stream(np.ascontiguousarray(x[part::w]), rate)[0] for part in range(w)]
    for exact in (True, False):
        r = api.Rs(taps, U, B, mode=L.RS_RESAMPLE, data_complex=cplx)
        r.set_exact(exact)
        r.set_algo(L.RS_ALGO_DIRECT)
        y = sc.resample_array(api, r, x, rate, chunk=3 * B)[0]
        for part in range(w):
            got, ref = y[part::w], refs[part]
            assert len(got) == len(ref) and len(got) > 0, (B, U, rate, len(ref), len(got))
            if exact:
                assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (B, U, rate, cplx)
            else:
                assert synth.rel_rms(got, ref) <= TOL, (B, U, rate, cplx)


# (complex, blksize, U, rate): calls dealt to 32 or 64 workgroups where the tile rule before csrc/segtile.h -- max_m / split +
# ceil(rate) + 64 + plen + 2 samples -- was short of a part's real span by 2 to 153 samples (tests/host/test_seg_split.cpp), and a
# complex call of 524288 samples that no split fits in 64 KiB: the host-scheduled path.  None of them leaves the reference in its
# out_len-exhausted state.
LARGE_SPLIT_SHAPES = [(True, 393216, 3, 1.0233), (True, 393216, 7, 0.77), (True, 393216, 2, 0.77), (True, 393216, 16, 0.77),
                      (False, 393216, 3, 1.0233), (False, 393216, 7, 1.77), (False, 524288, 3, 1.0233), (True, 524288, 3, 1.0233)]


def _rs_per_call(api, r, x, rate, B, w):
    """x (n_channels, w * n) through r, one reference call (B samples) per process_stream: (outputs, per-call counts)."""
    nch, n = x.shape[0], x.shape[1] // w
    cap = int(n / rate) + 4 * (n // B + 1) + 64
    d_in = sc.from_numpy(api, np.ascontiguousarray(x))
    d_out = sc.device_array(api, nch * w * cap)                                   # an output never stored stays NaN
    ks = []
    for off in range(0, n, B):
        m, k = min(B, n - off), sum(ks)
        ks.append(r.process_stream(d_in.ptr + 4 * w * off, m, d_out.ptr + 4 * w * k, cap - k, rate, in_stride=n, out_stride=cap))
    y = d_out.to_numpy().reshape(nch, w * cap)[:, : w * sum(ks)]
    d_in.free()
    d_out.free()
    return y, ks


@pytest.mark.timeout(600)
@pytest.mark.parametrize("plen", [32, 8])
@pytest.mark.parametrize("cplx,B,U,rate", LARGE_SPLIT_SHAPES)
def test_general_rate_split_calls_at_large_blksize(api, L, orc, cplx, B, U, rate, plen):
    """A call of the direct general-rate kernel larger than the LDS is dealt to up to 64 workgroups, each staging the input ITS
    outputs reach.  The float32 time law steps by a different amount in every binade, so equal runs of outputs reach unequal
    spans; the tile was sized max_m / split + a fixed slack and the kernel clamped a longer span to it, reading unstaged LDS with
    SFE_OK.  The tile is now the largest real span (csrc/segtile.h) or the call takes the host-scheduled path.  5 1/3 calls per
    stream.  Exact mode: the oracle's bits and ITS per-call output counts, one reference call per process_stream, then three;
    SFE_RS_ALGO_DIRECT in fused arithmetic and, at 8 taps per phase, the default algorithm (the direct kernel too: fewer than 12
    taps per phase): within 1e-5 and the same count.  Two channels on the first shape (blockIdx.y)."""
    rate = float(np.float32(rate))
    taps = synth.lowpass_taps(plen * U, 0.9 * min(1.0 / U, 1.0 / max(rate * U, 1.0)), gain=float(U))
    w = 2 if cplx else 1
    n = 5 * B + B // 3
    nch = 2 if (cplx, B, U, plen) == (True, 393216, 3, 32) else 1
    x = np.stack([synth.synth_f32(w * n, ch=150 + c) for c in range(nch)])
    refs, ref_ks = [], None
    for c in range(nch):
        for part in range(w):
            ref, ks = orc.Resample(taps, U, B).stream(np.ascontiguousarray(x[c, part::w]), rate)
            assert ref_ks is None or ks == ref_ks
            refs.append(ref)
            ref_ks = ks
    assert len(ref_ks) == 6 and min(ref_ks) > 0, ref_ks

    def check(y, exact, what):
        for c in range(nch):
            for part in range(w):
                got, ref = y[c, part::w], refs[c * w + part]
                assert len(got) == len(ref), (what, c, part, len(got), len(ref))
                if exact:
                    bad = np.flatnonzero(got.view(np.uint32) != ref.view(np.uint32))
                    assert bad.size == 0, (what, c, part, bad.size, bad[:8])
                else:
                    assert synth.rel_rms(got, ref) <= TOL, (what, c, part, synth.rel_rms(got, ref))

    def handle(exact, algo):
        r = api.Rs(taps, U, B, mode=L.RS_RESAMPLE, data_complex=cplx, n_channels=nch)
        r.set_exact(exact)
        if algo is not None:
            r.set_algo(algo)
        return r

    y, ks = _rs_per_call(api, handle(True, None), x, rate, B, w)
    assert ks == ref_ks, (ks, ref_ks)
    check(y, True, "exact, one call per process_stream")
    check(sc.resample_array(api, handle(True, None), x, rate, chunk=3 * B), True, "exact, three calls per process_stream")
    check(sc.resample_array(api, handle(False, L.RS_ALGO_DIRECT), x, rate, chunk=3 * B), False, "direct, fused")
    if plen == 8:
        check(sc.resample_array(api, handle(False, None), x, rate, chunk=3 * B), False, "default algorithm")


@pytest.mark.parametrize("U,step", [(9, 10), (24, 25), (10, 9), (32, 33), (16, 1), (32, 1), (12, 5), (64, 3), (9, 2), (160, 147), (147, 160), (256, 255), (100, 3)])
@pytest.mark.parametrize("cplx", [True, False])
def test_nine_to_sixty_four_outputs_per_period(api, L, orc, U, step, cplx):
    """Round 5 (poly_rt_dma.hip: poly_rt_dma_many_kernel): near-unity rate matching (10/9, 25/24, 33/32) and strong interpolation (x16, x32) -- 9 to
    64 outputs per period -- through the tiled form: the LDS-DMA tile, one m per thread, its phase sums eight at a time.  Within 1e-5 of the oracle
    (libdsp/resample.cxx:100-114 at an integer step) and BIT-IDENTICAL to the generic one-output-per-thread kernel, which still serves a stream
    off a 16-byte boundary (the same sums in the same order); two calls with carried state, three channels, an output off a 16-byte boundary."""
    taps = synth.lowpass_taps(24 * U - 1, 0.9 * min(1.0 / U, 1.0 / step), gain=float(U))
    rate = float(np.float32(step) / np.float32(U))
    w = 2 if cplx else 1
    n, nch = 3 * 4096 + 1235, 3
    x = np.stack([synth.synth_f32(w * n, ch=130 + c) for c in range(nch)])
    cap = n * U // step + 16
    cap += (-cap) % 4

    def run(offset_samples, stride, out_shift=0):
        buf = np.zeros(w * (offset_samples + stride * nch), np.float32)
        for c in range(nch):
            buf[w * (offset_samples + stride * c): w * (offset_samples + stride * c) + w * n] = x[c]
        d = sc.from_numpy(api, buf)
        d_out = sc.device_array(api, out_shift + w * cap * nch)
        r = api.Rs(taps, U, 4096, mode=L.RS_RESAMPLE, data_complex=cplx, n_channels=nch)
        r.set_algo(L.RS_ALGO_DIRECT)
        cut = 2 * 4096
        k1 = r.process_stream(d.ptr + 4 * w * offset_samples, cut, d_out.ptr + 4 * out_shift, cap, rate, in_stride=stride, out_stride=cap)
        k2 = r.process_stream(d.ptr + 4 * w * (offset_samples + cut), n - cut, d_out.ptr + 4 * (out_shift + w * k1), cap - k1, rate, in_stride=stride, out_stride=cap)
        return k1 + k2, d_out.to_numpy()[out_shift:].reshape(nch, w * cap)[:, : w * (k1 + k2)]

    al = (n + 3) // 4 * 4
    k, y = run(0, al)
    ku, yu = run(1, al + 1)
    assert k == ku and np.array_equal(y.view(np.uint32), yu.view(np.uint32)), (U, step, cplx)
    ko, yo = run(0, al, out_shift=w)
    assert k == ko and np.array_equal(y.view(np.uint32), yo.view(np.uint32)), (U, step, cplx)
    for part in range(w):
        ref = orc.Resample(taps, U, 4096).stream(np.ascontiguousarray(x[nch - 1, part::w]), rate)[0]
        sc.check_total(k, len(ref), n, U, rate)
        assert synth.rel_rms(y[nch - 1, part::w], ref) <= TOL, (U, step, cplx, part)


# ----------------------------------------------------------------- edge cases / misuse
def test_empty_and_tiny_inputs(api, L, orc):
    """n = 0 is a no-op; n < n_taps works and carries state; 1-tap filter is a gain."""
    taps = synth.taps_cfg2()
    f = api.Fir(taps, data_complex=True)
    d, d2 = sc.device_array(api, 16), sc.device_array(api, 16)
    f.process_stream(d, d2, 0)                      # nothing launched, no error
    x = synth.synth_cf32(600)
    parts = [sc.fir_filter(api, f, x[2 * a:2 * b])[0] for a, b in ((0, 1), (1, 3), (3, 200), (200, 600))]
    ref = oracle_fir_cf32(orc, taps, x)
    assert synth.rel_rms(np.concatenate(parts), ref) <= TOL
    g = api.Fir(np.array([0.5], np.float32), data_complex=False)
    xr = synth.synth_f32(5000)
    assert synth.rel_rms(sc.fir_filter(api, g, xr)[0], 0.5 * xr) <= 1e-6
    r = api.Rs(synth.taps_cfg4(), 1, 4096, mode=L.RS_DECIMATE)
    assert r.process_stream(d, 0, d2, 0, 8.0) == 0


def test_very_long_filter(api, L):
    """A quarter of a million taps: 120 partitions through the FFT kernel, still the streaming
    convolution; the time-domain kernel cannot hold such a filter and says so."""
    rng = np.random.default_rng(9)
    n_taps = 64 * 3840 + 5
    taps = (rng.standard_normal(n_taps) / 500).astype(np.float32)
    x = synth.synth_f32(300000)
    y = sc.fir_filter(api, api.Fir(taps, data_complex=False), x)[0]
    from scipy.signal import fftconvolve
    ref = fftconvolve(x.astype(np.float64), taps.astype(np.float64))[: len(x)]
    assert synth.rel_rms(y, ref) <= TOL
    f = api.Fir(taps, data_complex=False)
    f.set_algo(L.FIR_ALGO_DIRECT)
    with pytest.raises(api.SfeError):
        sc.fir_filter(api, f, x)


def test_misuse_is_reported_not_crashed(api, L):
    taps = synth.taps_cfg2()
    f = api.Fir(taps, data_complex=True)
    d = sc.device_array(api, 64)
    with pytest.raises(api.SfeError):               # in-place is not supported
        f.process_stream(d, d, 8)
    with pytest.raises(api.SfeError):               # host block path needs block_hint
        f.host_buffer()
    with pytest.raises(api.SfeError):               # fft_len too small for the taps (blkconv.cxx:47)
        api.Fir(taps, data_complex=False, block_hint=100)
    with pytest.raises(api.SfeError):
        api.Rs(taps, 0, 128)                        # upsample < 1
    r = api.Rs(taps, 4, 128, mode=L.RS_DECIMATE)
    with pytest.raises(api.SfeError):               # decimate rejects rate < 1 on the bulk path too
        r.process_stream(d, 8, sc.device_array(api, 64), 32, 0.5)
    ctaps = synth.complex_taps(64, 0.2)
    fc = api.Fir(ctaps[0] + 1j * ctaps[1], data_complex=True)
    fc.set_algo(L.FIR_ALGO_DIRECT)
    with pytest.raises(api.SfeError):               # complex taps need the FFT kernel
        sc.fir_filter(api, fc, synth.synth_cf32(1000))


def test_stale_handle_is_rejected(api, L):
    """A destroyed (or foreign) handle is reported, not dereferenced blindly."""
    import ctypes as C
    f = api.Fir(synth.taps_cfg2(), data_complex=True)
    h = f._h
    f.close()
    lib = L.load()
    buf = (C.c_char * 256)()              # a live allocation that is not a handle
    rc = lib.sfe_dsp_fir_reset(C.cast(buf, C.c_void_p))
    assert rc == L.SFE_EINVAL
    assert h is not None


def test_fir_tx10_output_fused(api, L, orc):
    """Pulse-shaping chain with the transmit converter fused into the store: the packed bytes
    equal oracle.tx_f32_to_10bit applied to the float output of the same kernel, bit for bit
    (sink_f_impl.cc:117-143), over chunked calls; only whole groups of 4 samples are emitted."""
    taps = synth.lowpass_taps(111, 0.2)
    n = 40000 + 3                                     # 3 trailing samples form no group
    x = (0.6 * synth.synth_f32(n)).astype(np.float32)
    yf = sc.fir_filter(api, api.Fir(taps, data_complex=False, algo=L.FIR_ALGO_FFT), x)[0]
    want = orc.tx_f32_to_10bit(yf)
    f = api.Fir(taps, data_complex=False, algo=L.FIR_ALGO_FFT)
    f.set_output_format(L.FMT_TX10)
    d_in = sc.from_numpy(api, x)
    d_out = sc.device_array(api, n // 4 * 5 // 4 + 8)
    d_out.zero()
    f.process_stream(d_in, d_out, n)
    got = d_out.to_numpy().view(np.uint8)[: n // 4 * 5]
    assert len(want) == n // 4 * 5 and np.array_equal(got, want)
    # chunked, chunk sizes multiples of 4 so groups line up across calls
    f.reset()
    outs = []
    for a, b in ((0, 4000), (4000, 4004), (4004, 20000), (20000, 40000)):
        d_i = sc.from_numpy(api, x[a:b])
        d_o = sc.device_array(api, (b - a) // 4 * 5 // 4 + 8)
        f.process_stream(d_i, d_o, b - a)
        outs.append(d_o.to_numpy().view(np.uint8)[: (b - a) // 4 * 5])
    got2 = np.concatenate(outs)
    # chunk seams move transform boundaries: codes may differ by 1 LSB where a sample sits on a step
    b5a, b5b = got2.reshape(-1, 5).astype(np.int32), want[: len(got2)].reshape(-1, 5).astype(np.int32)
    va = np.stack([((b5a[:, 0] >> (2 * k)) & 3) << 8 | b5a[:, 1 + k] for k in range(4)], 1)
    vb = np.stack([((b5b[:, 0] >> (2 * k)) & 3) << 8 | b5b[:, 1 + k] for k in range(4)], 1)
    assert np.abs(va - vb).max() <= 1 and np.count_nonzero(va != vb) <= 0.002 * va.size
    with pytest.raises(api.SfeError):                 # real data through complex taps: not built
        api.Fir(taps.astype(np.complex64), data_complex=False).set_output_format(L.FMT_TX10)


@pytest.mark.parametrize("n_taps", [2818, 3000, 3841])
def test_fir_tx10_for_a_filter_the_planner_would_partition(api, L, orc, n_taps):
    """~2818..3841 taps are served fastest by two partitions (sfe_dsp_fir_plan), and the 10-bit
    output exists for the single-launch kernel only.  Asking for TX10 re-plans such a handle as ONE
    partition (one transform can still overlap the filter) instead of failing; beyond 3841 taps it fails."""
    import ctypes as C
    ovl, parts, adv = C.c_int(0), C.c_int(0), C.c_int(0)
    api.check(L.load().sfe_dsp_fir_plan(n_taps, C.byref(ovl), C.byref(parts), C.byref(adv)))
    assert parts.value == 2
    taps = (synth.lowpass_taps(n_taps, 0.1) * 0.8).astype(np.float32)
    n = 60000
    x = (0.5 * synth.synth_f32(n, ch=4)).astype(np.float32)
    yf = np.convolve(x.astype(np.float64), taps.astype(np.float64))[:n].astype(np.float32)
    want = orc.tx_f32_to_10bit(yf)
    f = api.Fir(taps, data_complex=False, algo=L.FIR_ALGO_FFT)
    f.set_output_format(L.FMT_TX10)
    d_in = sc.from_numpy(api, x)
    d_out = sc.device_array(api, n // 4 * 5 // 4 + 8)
    d_out.zero()
    f.process_stream(d_in, d_out, n)
    got = d_out.to_numpy().view(np.uint8)[: n // 4 * 5]
    b5a, b5b = got.reshape(-1, 5).astype(np.int32), want.reshape(-1, 5).astype(np.int32)
    va = np.stack([((b5a[:, 0] >> (2 * k)) & 3) << 8 | b5a[:, 1 + k] for k in range(4)], 1)
    vb = np.stack([((b5b[:, 0] >> (2 * k)) & 3) << 8 | b5b[:, 1 + k] for k in range(4)], 1)
    assert np.abs(va - vb).max() <= 1 and np.count_nonzero(va != vb) <= 0.004 * va.size
    # and the float output of a re-planned handle still is the filter (switching back keeps the single plan)
    f.set_output_format(L.FMT_F32)
    f.reset()
    d_f = sc.device_array(api, n)
    f.process_stream(d_in, d_f, n)
    assert synth.rel_rms(d_f.to_numpy(), yf) <= TOL
    with pytest.raises(api.SfeError):
        api.Fir((synth.lowpass_taps(4100, 0.1)).astype(np.float32), data_complex=False).set_output_format(L.FMT_TX10)


@pytest.mark.parametrize("ctaps", [False, True])
def test_fir_tx10_output_fused_complex(api, L, orc, ctaps):
    """Complex stream with the transmit converter fused into the store
    (gr-simplefe/lib/sink_c_impl.cc:118-144: re, im, re, im -> 5 bytes): equals
    oracle.tx_f32_to_10bit over the interleaved float output of the same kernel, bit for bit;
    an odd trailing sample forms no group; two channels at their byte strides."""
    taps = synth.lowpass_taps(111, 0.2)
    if ctaps:
        taps = (taps * np.exp(1j * 0.3 * np.arange(len(taps)))).astype(np.complex64)
    n, nch = 30001, 2
    x = np.stack([(0.5 * synth.synth_cf32(n, ch=c)).astype(np.float32) for c in range(nch)])
    yf = sc.fir_filter(api, api.Fir(taps, data_complex=True, n_channels=nch, algo=L.FIR_ALGO_FFT), x)
    f = api.Fir(taps, data_complex=True, n_channels=nch, algo=L.FIR_ALGO_FFT)
    f.set_output_format(L.FMT_TX10)
    d_in = sc.from_numpy(api, x)
    stride = n + 1                                      # even: channel c at byte offset c*(stride/2)*5
    d_out = sc.device_array(api, nch * (stride // 2) * 5 // 4 + 8)
    d_out.zero()
    f.process_stream(d_in, d_out, n, in_stride=n, out_stride=stride)
    raw = d_out.to_numpy().view(np.uint8)
    for c in range(nch):
        want = orc.tx_f32_to_10bit(yf[c][: (n // 2) * 4])
        got = raw[c * (stride // 2) * 5: c * (stride // 2) * 5 + (n // 2) * 5]
        assert len(want) == (n // 2) * 5 and np.array_equal(got, want), c
    # the half group after the last whole one stays untouched
    assert not raw[(nch - 1) * (stride // 2) * 5 + (n // 2) * 5:][:5].any()


def _codes(b):
    b5 = np.asarray(b).reshape(-1, 5).astype(np.int32)
    return np.stack([((b5[:, 0] >> (2 * k)) & 3) << 8 | b5[:, 1 + k] for k in range(4)], 1)


@pytest.mark.parametrize("cplx", [True, False])
def test_fir_wire_to_wire_u8_in_tx10_out(api, L, orc, cplx):
    """The source_c -> FIR -> sink_c flowgraph in ONE launch: u8 offset-binary samples in
    (gr-simplefe/lib/source_c_impl.cc:121-132), 10-bit packed bytes out (sink_c_impl.cc:118-144;
    real streams: source_f_impl.cc:120-129 / sink_f_impl.cc:117-143).  Bit for bit the oracle's
    packing of the SAME kernel's float output; against the full oracle chain
    tx_f32_to_10bit(blkconv(rx_u8(bytes))) codes may differ by one LSB where a filtered sample
    sits on a quantiser step (the two float32 FFTs round differently), nowhere else."""
    taps = synth.lowpass_taps(111, 0.2)
    n = 50000 + (2 if cplx else 0)
    w = 2 if cplx else 1
    b = _u8_stream(n * w, 77)
    d_b = sc.from_bytes(api, b)
    # float output of the u8-input kernel
    f0 = api.Fir(taps, data_complex=cplx, algo=L.FIR_ALGO_FFT)
    f0.set_input_format(L.FMT_U8)
    d_f = sc.device_array(api, n * w)
    f0.process_stream(d_b, d_f, n)
    yf = d_f.to_numpy()
    # wire to wire
    f = api.Fir(taps, data_complex=cplx, algo=L.FIR_ALGO_FFT)
    f.set_input_format(L.FMT_U8)
    f.set_output_format(L.FMT_TX10)
    n_bytes = (n * w // 4) * 5
    d_o = sc.device_array(api, n_bytes // 4 + 8)
    d_o.zero()
    f.process_stream(d_b, d_o, n)
    got = d_o.to_numpy().view(np.uint8)[:n_bytes]
    assert np.array_equal(got, orc.tx_f32_to_10bit(yf[: (n * w // 4) * 4]))
    # the whole reference chain on the CPU
    xf = orc.rx_u8_to_cf32(b) if cplx else orc.rx_u8_to_f32(b)
    if cplx:
        ref = oracle_fir_cf32(orc, taps, xf)
    else:
        ref = orc.Blkconv(taps, 4096).stream(xf)
    want = orc.tx_f32_to_10bit(ref[: (n * w // 4) * 4])
    va, vb = _codes(got), _codes(want)
    assert np.abs(va - vb).max() <= 1 and np.count_nonzero(va != vb) <= 0.002 * va.size
    # a second call continues the stream (carried history is float32 converted from the bytes)
    f.process_stream(d_b, d_o, n)
    f0.process_stream(d_b, d_f, n)
    assert np.array_equal(d_o.to_numpy().view(np.uint8)[:n_bytes], orc.tx_f32_to_10bit(d_f.to_numpy()[: (n * w // 4) * 4]))


# ------------------------------------------- filters longer than one transform can overlap
@pytest.mark.parametrize("n_taps,cplx,nch", [(3000, True, 1), (3841, True, 1), (4096, True, 2), (8192, True, 1),
                                             (10000, False, 1), (5000, False, 3), (551, True, 1)])
def test_fir_long_filters_partitioned(api, L, n_taps, cplx, nch):
    """blkconv accepts any n_taps that leaves a block (blkconv.cxx:47; the reference's bpsk example
    offers a 551-tap prototype at fft 8192, examples/bpsk/bpsk.cxx:58-63).  Beyond what one
    4096-point transform can overlap usefully the tap vector is cut into partitions, one launch
    each, accumulated in the output (api_fir.hip fir_choose_partition).  Against the float64
    convolution; chunked calls shorter than the carried history exercise the unfused state update."""
    from scipy.signal import fftconvolve
    rng = np.random.default_rng(n_taps)
    taps = (rng.standard_normal(n_taps) / np.sqrt(n_taps)).astype(np.float32)
    n = 60000
    w = 2 if cplx else 1
    x = np.stack([(synth.synth_cf32(n, ch=c) if cplx else synth.synth_f32(n, ch=c)) for c in range(nch)])
    f = api.Fir(taps, data_complex=cplx, n_channels=nch, algo=L.FIR_ALGO_FFT)
    y = sc.fir_filter(api, f, x)
    for c in range(nch):
        for part in range(w):
            r64 = fftconvolve(x[c, part::w].astype(np.float64), taps.astype(np.float64))[:n]
            assert synth.rel_rms(y[c, part::w], r64) <= TOL, (c, part)
    # the same stream in ragged chunks (some shorter than the history): carried state
    f.reset()
    outs = []
    cuts = [0, 100, 4000, 4001, 30000, 52345, n]
    for a, b in zip(cuts[:-1], cuts[1:]):
        d_in = sc.from_numpy(api, np.ascontiguousarray(x[:, a * w: b * w]))
        d_out = sc.device_array(api, nch * (b - a) * w)
        f.process_stream(d_in, d_out, b - a)
        outs.append(d_out.to_numpy().reshape(nch, -1))
    y2 = np.concatenate(outs, axis=1)
    assert synth.rel_rms(y2, y) <= 2e-6


def test_fir_long_filter_u8_input_and_split(api, L):
    """A partitioned filter reads the u8 wire format too, and one stream cut into spans with
    load_history (history = parts x overlap samples) matches the uncut result."""
    from scipy.signal import fftconvolve
    rng = np.random.default_rng(5)
    taps = (rng.standard_normal(6000) / np.sqrt(6000)).astype(np.float32)
    n = 50000
    b = _u8_stream(2 * n, 3)
    xf = ((b.astype(np.float32) - 128.0) * np.float32(1.0 / 127.0))
    f = api.Fir(taps, data_complex=True, algo=L.FIR_ALGO_FFT)
    f.set_input_format(L.FMT_U8)
    d_out = sc.device_array(api, 2 * n)
    f.process_stream(sc.from_bytes(api, b), d_out, n)
    y = d_out.to_numpy()
    for part in (0, 1):
        assert synth.rel_rms(y[part::2], fftconvolve(xf[part::2].astype(np.float64), taps.astype(np.float64))[:n]) <= TOL
    with pytest.raises(api.SfeError):
        f.set_output_format(L.FMT_TX10)                  # packed output cannot be accumulated into
    g = api.Fir(taps, data_complex=True, algo=L.FIR_ALGO_FFT)
    cut = 23456
    g.load_history(sc.from_numpy(api, xf[2 * (cut - 6000): 2 * cut]), 6000)
    d2 = sc.device_array(api, 2 * (n - cut))
    g.process_stream(sc.from_numpy(api, xf[2 * cut:]), d2, n - cut)
    assert synth.rel_rms(d2.to_numpy(), y[2 * cut:]) <= 2e-6


@pytest.mark.parametrize("U,rate,blk,n_taps,mode", [(3, 5.0 / 3.0, 4096, 381, "resample"), (1, 8.0, 4096, 64, "decimate"),
                                                    (4, 1.77, 128, 31, "resample"), (4, 0.77, 128, 31, "resample")])
def test_rs_pipe_equals_the_reference_stream(api, L, orc, U, rate, blk, n_taps, mode):
    """sfe_dsp_rs_pipe_*: scheduler-sized pushes, pinned batches of whole blksize-sample reference
    calls, four in flight.  What comes out of pull -- in order, nothing lost at the end -- is bit for
    bit what the reference object produces when fed the stream blksize samples at a time
    (resample.cxx:85-153), for integer-valued and general rates alike."""
    import ctypes as C
    rng = np.random.default_rng(int(rate * 100))
    taps = (rng.standard_normal(n_taps) / np.sqrt(n_taps) * U).astype(np.float32)
    n = 150001
    x = synth.synth_f32(n, ch=11)
    r = api.Rs(taps, U, blk, mode=L.RS_RESAMPLE if mode == "resample" else L.RS_DECIMATE)
    r.set_exact(True)
    lib = L.load()
    p = C.c_void_p()
    api.check(lib.sfe_dsp_rs_pipe_create(r._h, 10000, rate, C.byref(p)))       # rounded up to whole blksize calls
    out = np.zeros(int(n / min(rate, 1e9)) + 4096, np.float32)
    taken, got = C.c_size_t(0), C.c_size_t(0)
    off = k = 0
    sizes = [4096, 1000, 8191, 37, 16384]
    i = 0
    while off < n:
        m = min(sizes[i % 5], n - off)
        i += 1
        api.check(lib.sfe_dsp_pipe_push(p, x.ctypes.data + 4 * off, m, C.byref(taken)))
        off += taken.value
        api.check(lib.sfe_dsp_pipe_pull(p, out.ctypes.data + 4 * k, 5000, 0 if taken.value else 1, C.byref(got)))
        k += got.value
    while True:                                                                # drain
        api.check(lib.sfe_dsp_pipe_pull(p, out.ctypes.data + 4 * k, 5000, 2, C.byref(got)))
        if got.value == 0:
            break
        k += got.value
    lib.sfe_dsp_pipe_destroy(p)
    ref, _ = getattr(orc, "Resample" if mode == "resample" else "Decimate")(taps, U, blk).stream(x, rate)
    sc.check_total(k, len(ref), n, U, rate)
    assert np.array_equal(out[:k], ref)


def test_pipe_without_host_copies_equals_push_and_pull(api, L):
    """sfe_dsp_pipe_acquire / commit / peek / release: the producer writes into the pipe's pinned batch, the consumer
    reads finished items in place (blkconv.h:44-47's get_process_buf() idea).  Same items in the same order as push /
    pull, also when the two forms are mixed on one pipe; room and availability are enforced."""
    import ctypes as C
    lib = L.load()
    taps = synth.taps_cfg2()
    n = 300001
    x = synth.synth_cf32(n, ch=5)

    def run(mixed, copies=False):
        f = api.Fir(taps, data_complex=True)
        p = C.c_void_p()
        api.check(lib.sfe_dsp_fir_pipe_create(f._h, 16384, C.byref(p)))
        out = np.zeros(n, np.complex64)
        buf, room, got, taken = C.c_void_p(), C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        src = C.c_void_p()
        off = k = i = 0
        sizes = [4096, 1000, 8191, 37, 20000]

        def take(wait):
            nonlocal k
            if copies:
                api.check(lib.sfe_dsp_pipe_pull(p, out.ctypes.data + 8 * k, 5000, wait, C.byref(got)))
                k += got.value
                return got.value
            api.check(lib.sfe_dsp_pipe_peek(p, C.byref(src), C.byref(got), wait))
            if got.value:
                m = got.value if not mixed or (k & 1) == 0 else max(1, got.value // 3)      # partial releases too
                out[k:k + m] = np.frombuffer((C.c_char * (8 * m)).from_address(src.value), np.complex64)
                api.check(lib.sfe_dsp_pipe_release(p, m))
                k += m
            return got.value

        while off < n:
            want = min(sizes[i % 5], n - off)
            i += 1
            if copies or (mixed and i % 3 == 0):
                api.check(lib.sfe_dsp_pipe_push(p, x.ctypes.data + 8 * off, want, C.byref(taken)))
                off += taken.value
                moved = taken.value
            else:
                api.check(lib.sfe_dsp_pipe_acquire(p, C.byref(buf), C.byref(room)))
                moved = min(want, room.value)
                if moved:
                    C.memmove(buf.value, x.ctypes.data + 8 * off, 8 * moved)
                    api.check(lib.sfe_dsp_pipe_commit(p, moved))
                    off += moved
            take(0 if moved else 1)
        while take(2):
            pass
        # the contracts: nothing to release, nothing beyond the reported room
        assert lib.sfe_dsp_pipe_release(p, 1) == L.SFE_EINVAL
        api.check(lib.sfe_dsp_pipe_acquire(p, C.byref(buf), C.byref(room)))
        assert room.value == 16384 and lib.sfe_dsp_pipe_commit(p, room.value + 1) == L.SFE_EINVAL
        lib.sfe_dsp_pipe_destroy(p)
        f.close()
        assert k == n
        return out

    f = api.Fir(taps, data_complex=True)
    bulk = sc.fir_filter(api, f, x.view(np.float32)).reshape(-1).view(np.complex64)
    f.close()
    ref = run(False, copies=True)          # push / pull: the same batches, hence the same transform positions and the same bits
    assert np.array_equal(run(False), ref) and np.array_equal(run(True), ref)
    assert np.sqrt(np.sum(np.abs(ref - bulk) ** 2) / np.sum(np.abs(bulk) ** 2)) < 1e-6      # (one bulk call cuts its transforms elsewhere)


@pytest.mark.parametrize("cplx", [True, False])
def test_fir_pipe_takes_the_u8_wire_format(api, L, orc, cplx):
    """sfe_dsp_fir_pipe_* over a handle whose input format is the receive wire format: u8 items in (2 bytes per
    complex item, gr-simplefe/lib/source_c_impl.cc:121-132), float32 items out, scheduler-sized pushes.
    Bit for bit the bulk device call on the same bytes, and within the bar of the oracle's conversion + filter."""
    import ctypes as C
    rng = np.random.default_rng(5)
    n = 300001
    per = 2 if cplx else 1
    raw = rng.integers(0, 256, size=per * n, dtype=np.uint8)
    taps = synth.taps_cfg2()
    f = api.Fir(taps, data_complex=cplx)
    f.set_input_format(L.FMT_U8)
    lib = L.load()
    p = C.c_void_p()
    api.check(lib.sfe_dsp_fir_pipe_create(f._h, 1 << 16, C.byref(p)))
    # the pipe froze the handle's item formats -- switching them (the pipe's device batches hold
    # 1-2 bytes per item) or destroying the handle under the pipe is refused, not undefined
    assert lib.sfe_dsp_fir_set_input_format(f._h, L.FMT_F32) == L.SFE_ESTATE
    assert lib.sfe_dsp_fir_set_output_format(f._h, L.FMT_TX10) == L.SFE_ESTATE
    assert lib.sfe_dsp_fir_set_input_format(f._h, L.FMT_U8) == L.SFE_OK            # unchanged format: fine
    assert lib.sfe_dsp_fir_destroy(f._h) == L.SFE_ESTATE
    out = np.zeros(per * n, np.float32)
    taken, got = C.c_size_t(0), C.c_size_t(0)
    off = k = 0
    sizes = [4096, 1001, 8191, 37, 16384]
    i = 0
    while off < n:
        m = min(sizes[i % 5], n - off)
        i += 1
        api.check(lib.sfe_dsp_pipe_push(p, raw.ctypes.data + per * off, m, C.byref(taken)))
        off += taken.value
        api.check(lib.sfe_dsp_pipe_pull(p, out.ctypes.data + 4 * per * k, 6000, 0 if taken.value else 1, C.byref(got)))
        k += got.value
    while True:
        api.check(lib.sfe_dsp_pipe_pull(p, out.ctypes.data + 4 * per * k, 6000, 2, C.byref(got)))
        if got.value == 0:
            break
        k += got.value
    lib.sfe_dsp_pipe_destroy(p)
    assert lib.sfe_dsp_fir_set_input_format(f._h, L.FMT_F32) == L.SFE_OK           # released with the pipe
    assert k == n
    # the bulk call on the same bytes, cut where the pipe cut its batches (the FFT kernel's results do not depend on the cut)
    g = api.Fir(taps, data_complex=cplx)
    g.set_input_format(L.FMT_U8)
    d_in, d_out = sc.from_bytes(api, raw), sc.device_array(api, per * n)
    g.process_stream(d_in, d_out, n)
    bulk = d_out.to_numpy(per * n)
    assert synth.rel_rms(out, bulk) <= 2e-6
    xf = orc.rx_u8_to_cf32(raw) if cplx else orc.rx_u8_to_f32(raw)
    for part in range(per):
        ref = orc.Blkconv(taps, 4096).stream(np.ascontiguousarray(xf[part::per]))
        assert synth.rel_rms(out[part::per], ref) <= TOL


def test_rs_pipe_takes_the_u8_wire_format(api, L, orc, g5):
    """sfe_dsp_rs_pipe_* over a decimate-by-8 handle reading the receive wire format (`source_c -> decimate`):
    u8 items in (2 bytes per complex item), cf32 items out, scheduler-sized pushes; within the bar of
    converter -> oracle, nothing lost at the end."""
    import ctypes as C
    taps, U, rate = g5["cfg4_taps"], int(g5["cfg4_U"]), float(g5["cfg4_rate"])
    n = 200000
    raw = _u8_stream(2 * n, 3)
    r = api.Rs(taps, U, 4096, mode=L.RS_RESAMPLE, data_complex=True)
    r.set_input_format(L.FMT_U8)
    lib = L.load()
    p = C.c_void_p()
    api.check(lib.sfe_dsp_rs_pipe_create(r._h, 1 << 15, rate, C.byref(p)))
    assert lib.sfe_dsp_rs_set_input_format(r._h, L.FMT_F32) == L.SFE_ESTATE        # frozen by the pipe
    assert lib.sfe_dsp_rs_destroy(r._h) == L.SFE_ESTATE
    out = np.zeros(2 * (int(n / rate) + 4096), np.float32)
    taken, got = C.c_size_t(0), C.c_size_t(0)
    off = k = i = 0
    sizes = [4096, 1001, 8191, 37, 16384]
    while off < n:
        m = min(sizes[i % 5], n - off)
        i += 1
        api.check(lib.sfe_dsp_pipe_push(p, raw.ctypes.data + 2 * off, m, C.byref(taken)))
        off += taken.value
        api.check(lib.sfe_dsp_pipe_pull(p, out.ctypes.data + 8 * k, 3000, 0 if taken.value else 1, C.byref(got)))
        k += got.value
    while True:
        api.check(lib.sfe_dsp_pipe_pull(p, out.ctypes.data + 8 * k, 3000, 2, C.byref(got)))
        if got.value == 0:
            break
        k += got.value
    lib.sfe_dsp_pipe_destroy(p)
    xf = orc.rx_u8_to_f32(raw)
    for part in (0, 1):
        ref, _ = orc.Resample(taps, U, 4096).stream(np.ascontiguousarray(xf[part::2]), rate)
        sc.check_total(k, len(ref), n, U, rate)
        assert synth.rel_rms(out[part:2 * k:2], ref) <= TOL


def test_stream_entry_points_reject_bad_buffers(api, L):
    """sfe_dsp_rs_process_stream has the checks the FIR entry has -- channel strides that
    would let channels overwrite each other, pointers not aligned to their element, input and
    output ranges that overlap (partially, not only d_in == d_out) -- and returns SFE_EINVAL before
    anything is launched; the FIR entry rejects partial overlap too."""
    import ctypes as C
    lib = L.load()
    taps = synth.taps_cfg4()
    buf = sc.device_array(api, 1 << 16)
    n_out = C.c_size_t(0)

    def rs_call(r, d_in, n_in, in_stride, d_out, out_cap, out_stride):
        return lib.sfe_dsp_rs_process_stream(r._h, d_in, n_in, in_stride, d_out, out_cap, out_stride, 8.0, C.byref(n_out), None)
    r2 = api.Rs(taps, 1, 4096, mode=L.RS_DECIMATE, data_complex=True, n_channels=2)
    base = buf.ptr
    assert rs_call(r2, base, 4096, 4000, base + (1 << 17), 600, 600) == L.SFE_EINVAL      # in_stride < n_in
    assert rs_call(r2, base, 4096, 4096, base + (1 << 17), 600, 520) == L.SFE_EINVAL      # out_stride < out_cap
    assert rs_call(r2, base + 4, 4096, 4096, base + (1 << 17), 600, 600) == L.SFE_EINVAL  # cf32 input not 8-byte aligned
    assert rs_call(r2, base, 4096, 4096, base + (1 << 17) + 4, 600, 600) == L.SFE_EINVAL  # output not aligned
    assert rs_call(r2, base, 4096, 4096, base + 8 * 8000, 600, 600) == L.SFE_EINVAL       # output starts inside the input range
    assert rs_call(r2, base, 4096, 4096, base, 600, 600) == L.SFE_EINVAL                  # same buffer
    assert rs_call(r2, base, 4096, 4096, base + (1 << 17), 600, 600) == L.SFE_OK and n_out.value == 512
    f = api.Fir(synth.taps_cfg2(), data_complex=True)
    assert lib.sfe_dsp_fir_process_stream(f._h, base, base + 8 * 1000, 4096, 4096, 4096, None) == L.SFE_EINVAL   # partial overlap
    assert lib.sfe_dsp_fir_process_stream(f._h, base + 2, base + (1 << 17), 4096, 4096, 4096, None) == L.SFE_EINVAL
    assert b"overlap" in lib.sfe_dsp_last_error() or b"aligned" in lib.sfe_dsp_last_error()
    assert lib.sfe_dsp_fir_process_stream(f._h, base, base + (1 << 17), 4096, 4096, 4096, None) == L.SFE_OK
    api.sync()


def test_fir_per_channel_taps_ticket_groups_by_channel(api, L):
    """Sixteen channels (a multiple of the eight ticket groups) with more transforms than resident workgroups: the launch
    deals each group whole channels (FirFftArgs::ch_groups) -- every channel against a single-channel handle
    with that channel's taps (the same transform arithmetic: identical bits), two calls, state carried."""
    rng = np.random.default_rng(16)
    nch, n = 16, 330000                     # 86 transforms per channel: 1376 tickets for ~1024 workgroups
    taps = rng.standard_normal((nch, 256)).astype(np.float32) / 16.0
    x = np.stack([synth.synth_cf32(n, ch=40 + c) for c in range(nch)])
    d_in = sc.from_numpy(api, x)
    d_out = sc.device_array(api, nch * 2 * n)
    f = api.Fir(taps, per_channel=True)
    cut = 200000
    f.process_stream(d_in, d_out, cut, in_stride=n, out_stride=n)
    f.process_stream(d_in.ptr + 8 * cut, d_out.ptr + 8 * cut, n - cut, in_stride=n, out_stride=n)
    y = d_out.to_numpy().reshape(nch, 2 * n)
    for c in range(nch):
        one = api.Fir(taps[c], data_complex=True, algo=L.FIR_ALGO_FFT)
        a = sc.fir_filter(api, one, x[c, : 2 * cut])[0]
        b = sc.fir_filter(api, one, x[c, 2 * cut:])[0]
        assert np.array_equal(y[c], np.concatenate([a, b])), c
