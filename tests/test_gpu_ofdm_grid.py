"""Every class of the OFDM receiver's kernel on the GPU -- ofdm_kernel<log2 N 6 .. 12, u8 or cf32> -- over
ofdm_cases.GRID, whose shapes use every bin, so that the whole of every transform is compared: symbols per burst and per
data symbol's row, the channel estimate and the record against the float64 plan, the u8 path against the cf32 path's
bits, the exact case at the sizes the older file leaves out, a burst of 1024 data symbols that puts the float64 turn
count under load, and multi-stream calls at the two four-wave sizes that were never launched.  All through the guarded
buffers of tests/ofdm_run.py."""
import numpy as np
import pytest

import ofdm_cases as oc
from ofdm_run import _bits, run, same
from simplefe_amd import synth

pytestmark = pytest.mark.gpu
F32 = np.float32
SYM_BAR = 1e-5                      # rel-RMS: the project's bar for a float32 transform block against float64
EPS_ULPS = 4                        # the device's eps against the reference's own, in float32 ulps of the latter (seen: 0 and 1)


@pytest.fixture(scope="module")
def api():
    from simplefe_amd import api as a
    return a


@pytest.fixture(scope="module")
def L():
    from simplefe_amd import lib
    return lib


def record_close(got, want):
    d = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))
    return d, bool((d <= 1e-5 + 1e-4 * np.abs(np.asarray(want, np.float64))).all())


@pytest.mark.parametrize("out_mode", [0, 1], ids=["zf", "mrc"])
@pytest.mark.parametrize("name", oc.GRID_NAMES)
def test_symbols_chan_and_record_against_the_float64_plan(api, name, out_mode):
    """Per burst AND per data symbol's row: symbols within 1e-5 rel-RMS of the plan; chan within 1e-5; record words within
    1e-5 + 1e-4 |want|; null bins of chan and the record's reserved words are zero bits."""
    x, starts, sent = oc.stream(name)
    a = oc.shape_args(name, out_mode)
    want = api.ofdm_plan(x=x, idx=starts.astype(np.uint32), **a)
    h = api.Ofdm(**a)
    sym, ch, rec, st = (v[0] for v in run(api, h, x, len(starts), idx=starts, out_pad=3, st_pad=2, lead=1))
    h.close()
    assert not st.any() and not want[3].any()
    used = a["kind"] != 0
    for b in range(len(starts)):
        rows = [oc.rel_rms(sym[b, j], want[0][b, j]) for j in range(sym.shape[1])]
        es, ec = oc.rel_rms(sym[b], want[0][b]), oc.rel_rms(ch[b, used], want[1][b, used])
        d, ok = record_close(rec[b], want[2][b])
        print("%s burst %d: symbols %.2e (worst row %.2e) chan %.2e rel-RMS of %.0e; record |diff| %s"
              % (name, b, es, max(rows), ec, SYM_BAR, " ".join("%.1e" % v for v in d[:6])))
        assert es <= SYM_BAR and ec <= SYM_BAR and max(rows) <= SYM_BAR
        assert ok, d
        assert not _bits(rec[b, 6:]).any() and not _bits(ch[b, ~used]).any()


@pytest.mark.parametrize("name", oc.GRID_NAMES)
def test_u8_input_gives_the_bits_of_the_converted_samples(api, L, name):
    """The bytes at an address that is 2 mod 4; the cf32 path's symbols on the converted samples against the plan."""
    x0, starts, _ = oc.stream(name)
    n_bursts, step, R = 3, 21, oc.reach(name)
    x = x0[int(starts[0]):int(starts[0]) + R + (n_bursts - 1) * step]
    x = x * (0.7 / np.abs(x.view(F32)).max())
    by = np.clip(np.rint(x.view(F32).astype(np.float64) * 127.0 + 128.0), 0, 255).astype(np.uint8)
    a = oc.shape_args(name, 0)
    h = api.Ofdm(**a)
    want = run(api, h, synth.u8_to_cf32(by), n_bursts, start_step=step)
    h.set_input_format(L.FMT_U8)
    got = run(api, h, by, n_bursts, start_step=step, lead=1)
    h.close()
    assert want[3].tolist() == [[0] * n_bursts] and same(want, got)
    plan = api.ofdm_plan(x=synth.u8_to_cf32(by), n_bursts=1, **a)
    rows = [oc.rel_rms(want[0][0, 0, j], plan[0][0, j]) for j in range(plan[0].shape[1])]
    print("%s: cf32 path on the converted bytes, worst row %.2e of %.0e" % (name, max(rows), SYM_BAR))
    assert not plan[3].any() and oc.rel_rms(want[0][0, 0], plan[0][0]) <= SYM_BAR and max(rows) <= SYM_BAR


@pytest.mark.parametrize("name", ["g256", "g1024", "g2048"])
def test_the_exact_case_is_exact(api, name):
    """An impulse at every window's first sample, train of ones, every bin used: ones to the bit at the sizes the older
    file's exact case leaves out."""
    a, x, starts = oc.exact_case(name)
    used = a["kind"] != 0
    assert used.all()
    for out_mode in (0, 1):
        h = api.Ofdm(out_mode=out_mode, **a)
        sym, ch, rec, st = (v[0] for v in run(api, h, x, len(starts), idx=starts, out_pad=1, lead=3))
        h.close()
        assert not st.any()
        assert np.array_equal(_bits(sym), _bits(np.ones_like(sym)))
        assert np.array_equal(_bits(ch), _bits(np.ones_like(ch)))
        assert np.array_equal(_bits(rec), _bits(np.tile(np.array([0, 1, 1, 0, 0, 0, 0, 0], F32), (len(st), 1))))


@pytest.mark.parametrize("out_mode", [0, 1], ids=["zf", "mrc"])
@pytest.mark.parametrize("name", oc.LONG_NAMES)
def test_the_long_burst_row_by_row(api, name, out_mode):
    """1024 data symbols at eps = 0.4 and -0.47: the turn count eps n / N reaches 500 turns.  The device's eps is held
    within EPS_ULPS float32 ulps of the reference's own -- a margin set before any measurement, for an estimate that is a
    float32 sum of some 16 000 products through atan2f -- and then every row is held to
    synth.ofdm_reference(eps = the device's), the float64 law behind the same float32 hand-over, at 1e-5 rel-RMS, and the
    record at its usual bar.  A turn count formed in float32 puts row 512 at 6.9e-5 and the last rows at 1.4e-4 to 1.8e-4
    (numpy, the same eps); the float64 law sits at 2.7e-8."""
    x, starts, sent = oc.stream(name)
    a = oc.shape_args(name, out_mode)
    own = oc.reference(name, out_mode)[2][0, 0]
    h = api.Ofdm(**a)
    sym, ch, rec, st = (v[0, 0] for v in run(api, h, x, 1, idx=starts, out_pad=2, lead=1))
    h.close()
    assert st == 0
    ulps = abs(float(rec[0]) - float(own)) / float(np.spacing(np.abs(own)))
    print("%s: device eps %.9g, the reference's own %.9g: %.1f ulps of %d" % (name, rec[0], own, ulps, EPS_ULPS))
    assert ulps <= EPS_ULPS
    wsym, wch, wrec, wst = synth.ofdm_reference(x, int(starts[0]), eps=rec[0], **oc.reference_args(name, out_mode))
    assert wst == 0 and _bits(wrec[:1]) == _bits(rec[:1])
    rows = np.array([oc.rel_rms(sym[j], wsym[j]) for j in range(wsym.shape[0])])
    used = a["kind"] != 0
    d, ok = record_close(rec, wrec)
    print("%s: rows worst %.2e (row %d), row 512 %.2e, last %.2e, all %.2e, chan %.2e of %.0e; record |diff| %s"
          % (name, rows.max(), rows.argmax(), rows[512], rows[-1], oc.rel_rms(sym, wsym), oc.rel_rms(ch[used], wch[used]), SYM_BAR,
             " ".join("%.1e" % v for v in d[:6])))
    assert rows.max() <= SYM_BAR and oc.rel_rms(ch[used], wch[used]) <= SYM_BAR
    assert ok, d
    assert not _bits(rec[6:]).any() and not _bits(ch[~used]).any()
    assert np.array_equal(np.sign(sym.real), np.sign(sent[0].real)) and np.array_equal(np.sign(sym.imag), np.sign(sent[0].imag))


@pytest.mark.parametrize("name", ["g1024", "g2048"])
def test_two_streams_of_three_bursts_depend_on_their_reach_alone(api, name):
    """One call of 2 streams x 3 bursts at the four-wave sizes: windows 37 samples apart overlap, an index table jitters
    them, every stride is wider than its payload; the call twice, and every burst against a one-burst call of a
    one-stream handle at another input address, output address and stride, bit for bit."""
    n_streams, n_bursts = 2, 3
    x0, starts, _ = oc.stream(name)
    R, step = oc.reach(name), 37
    n = 11 + R + (n_bursts - 1) * step + 9
    x = np.stack([x0[s * 5:s * 5 + n] for s in range(n_streams)])      # bursts of sorts: any window will do
    rng = np.random.default_rng(5)
    jit = rng.integers(0, 9, size=(n_streams, n_bursts)).astype(np.uint32)
    a = oc.shape_args(name, 1)
    h = api.Ofdm(n_streams=n_streams, **a)
    kw = dict(idx=jit, start_base=3, start_step=step, out_pad=3, st_pad=2, lead=1, in_pad=5)
    u, v = run(api, h, x, n_bursts, **kw), run(api, h, x, n_bursts, **kw)
    h.close()
    assert not u[3].any() and same(u, v)
    one = api.Ofdm(**a)
    for s in range(n_streams):
        for bi in range(n_bursts):
            o = 3 + bi * step + int(jit[s, bi])
            cut = o - (bi % 3)
            got = run(api, one, x[s, cut:o + R], 1, start_base=o - cut, out_pad=bi % 5, lead=2 + bi % 4, chan=bool(bi & 1))
            for i in (0, 2, 3) + ((1,) if bi & 1 else ()):
                assert np.array_equal(_bits(u[i][s, bi]), _bits(got[i][0, 0])), (s, bi, i)
    one.close()
