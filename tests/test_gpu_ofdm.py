"""The OFDM burst receiver (sfe_dsp_ofdm_*) on the GPU: symbols, channel estimate and record against the float64 plan,
the promises about bits checked literally through guarded buffers, failed bursts, process_stream's refusals, a captured
call, and the chain Ldpc.encode_stream -> waveform -> Corr -> Ofdm -> Ldpc.process_stream with only handles, pointers and
strides between the device blocks."""
import ctypes as C

import numpy as np
import pytest

import ldpc_cases as lc
import ofdm_cases as oc
from ofdm_run import SENT, Run, _bits, run, same
from simplefe_amd import synth

pytestmark = pytest.mark.gpu
F32 = np.float32
SYM_BAR = 1e-5                      # rel-RMS per burst: the project's bar for a float32 transform block against float64


@pytest.fixture(scope="module")
def api():
    from simplefe_amd import api as a
    return a


@pytest.fixture(scope="module")
def L():
    from simplefe_amd import lib
    return lib


def hip_runtime():
    hip = C.CDLL("libamdhip64.so")
    for name, args in (("hipStreamCreate", [C.POINTER(C.c_void_p)]), ("hipStreamBeginCapture", [C.c_void_p, C.c_int]),
                       ("hipStreamEndCapture", [C.c_void_p, C.POINTER(C.c_void_p)]),
                       ("hipGraphInstantiate", [C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
                       ("hipGraphLaunch", [C.c_void_p, C.c_void_p]), ("hipStreamSynchronize", [C.c_void_p]),
                       ("hipGraphExecDestroy", [C.c_void_p]), ("hipGraphDestroy", [C.c_void_p]), ("hipStreamDestroy", [C.c_void_p])):
        fn = getattr(hip, name)
        fn.argtypes, fn.restype = args, C.c_int
    return hip


@pytest.mark.parametrize("out_mode", [0, 1], ids=["zf", "mrc"])
@pytest.mark.parametrize("name", oc.NAMES)
def test_symbols_chan_and_record_against_the_float64_plan(api, name, out_mode):
    """Per burst: symbols and chan within 1e-5 rel-RMS of the plan, record words within 1e-5 + 1e-4 |want|."""
    x, starts, sent = oc.stream(name)
    a = oc.shape_args(name, out_mode)
    want = api.ofdm_plan(x=x, idx=starts.astype(np.uint32), **a)
    h = api.Ofdm(**a)
    sym, ch, rec, st = (v[0] for v in run(api, h, x, len(starts), idx=starts, out_pad=3, st_pad=2, lead=1))
    h.close()
    assert not st.any() and not want[3].any()
    used = a["kind"] != 0
    for b in range(len(starts)):
        es, ec = oc.rel_rms(sym[b], want[0][b]), oc.rel_rms(ch[b, used], want[1][b, used])
        d = np.abs(rec[b].astype(np.float64) - want[2][b])
        print("%s burst %d: symbols %.2e chan %.2e rel-RMS of %.0e; record |diff| %s" % (name, b, es, ec, SYM_BAR, " ".join("%.1e" % v for v in d[:6])))
        assert es <= SYM_BAR and ec <= SYM_BAR
        assert (d <= 1e-5 + 1e-4 * np.abs(want[2][b].astype(np.float64))).all(), d
        assert not _bits(rec[b, 6:]).any() and not _bits(ch[b, ~used]).any()


@pytest.mark.parametrize("name", ["n64", "n128", "n4096"])
@pytest.mark.parametrize("n_streams,n_bursts", [(1, 1), (2, 5)])
def test_runs_repeat_and_a_burst_depends_on_its_reach_alone(api, name, n_streams, n_bursts):
    """The same call twice; every burst of the call against a one-burst call of a one-stream handle at another input
    address, output address and stride, without an index table and without d_chan; windows 37 samples apart overlap."""
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


@pytest.mark.parametrize("name", oc.NAMES)
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
    assert not plan[3].any() and oc.rel_rms(want[0][0, 0], plan[0][0]) <= SYM_BAR


@pytest.mark.parametrize("name", oc.NAMES)
def test_the_exact_case_is_exact(api, name):
    a, x, starts = oc.exact_case(name)
    used = a["kind"] != 0
    for out_mode in (0, 1):
        h = api.Ofdm(out_mode=out_mode, **a)
        sym, ch, rec, st = (v[0] for v in run(api, h, x, len(starts), idx=starts))
        h.close()
        assert not st.any()
        assert np.array_equal(_bits(sym), _bits(np.ones_like(sym)))
        assert np.array_equal(_bits(ch[:, used]), _bits(np.ones_like(ch[:, used]))) and not _bits(ch[:, ~used]).any()
        assert np.array_equal(_bits(rec), _bits(np.tile(np.array([0, 1, 1, 0, 0, 0, 0, 0], F32), (len(st), 1))))


def _failed(r, b):
    sym, ch, rec = r[0][0], r[1][0], r[2][0]
    return (not _bits(sym[b]).any() and not _bits(ch[b]).any() and np.isnan(rec[b, :6]).all()
            and ((_bits(rec[b, :6]) & 0x7fc00000) == 0x7fc00000).all() and not _bits(rec[b, 6:]).any())


@pytest.mark.parametrize("name", ["n64", "n512"])
def test_failed_bursts_get_the_stated_bits_and_leave_their_neighbours_alone(api, name):
    """Of eight bursts one holds a NaN sample, one an infinite one in no window, one is gated, one has a NaN gate, one starts
    beyond the buffer, one has silent training symbols (H = 0); the rest equal a call without any of that.  Then the
    range's two edges, one sample each way."""
    sh = oc.SHAPES[name]
    x0, starts, _ = oc.stream(name)
    R, Lsym = oc.reach(name), sh["n_fft"] + sh["cp"]
    nb, step = 8, R + 3
    burst = x0[int(starts[0]):int(starts[0]) + R]
    x = np.zeros(nb * step + 4, np.complex64)
    for b in range(nb):
        x[2 + b * step:2 + b * step + R] = burst
    a = oc.shape_args(name, 0, min_gate=0.5)
    h = api.Ofdm(**a)
    clean = run(api, h, x, nb, start_base=2, start_step=step)
    bad = x.copy()
    bad[2 + 1 * step] = complex(np.nan, 0.0)                    # burst 1: the first sample of its reach
    bad[2 + 3 * step + R - 1] = complex(0.0, np.inf)            # burst 3: the last one, behind every window
    bad[2 + 6 * step:2 + 6 * step + sh["n_train"] * Lsym] = 0   # burst 6: no training symbols: H = 0 on every used bin
    gate = np.array([1, 1, 0.25, 1, np.nan, 1, 1, 0.5], F32)
    idx = np.zeros(nb, np.uint32)
    idx[5] = 2 ** 32 - 5 * step - 3                             # burst 5 starts at o = 2^32 - 1: far beyond the buffer
    r = run(api, h, bad, nb, idx=idx, gate=gate, start_base=2, start_step=step)
    assert not clean[3].any() and r[3][0].tolist() == [0, 1, 2, 1, 2, 3, 1, 0]
    for b in range(nb):
        if r[3][0, b]:
            assert _failed(r, b), b
        else:
            assert all(np.array_equal(_bits(r[i][0, b]), _bits(clean[i][0, b])) for i in range(3)), b
    seg = x[2:2 + R]
    assert run(api, h, seg, 1)[3].tolist() == [[0]]
    assert run(api, h, seg, 2, start_base=-1, start_step=2)[3].tolist() == [[3, 3]]
    assert run(api, h, x[2:2 + R + 1], 2, start_step=1)[3].tolist() == [[0, 0]]
    assert run(api, h, seg, 1, start_base=-2 ** 40)[3].tolist() == [[3]]
    h.close()


def test_refusals_launch_nothing(api, L):
    name = "n64"
    S, nb = 2, 3
    x0, starts, _ = oc.stream(name)
    R = oc.reach(name)
    n = R + 8
    x = np.stack([x0[int(starts[0]):][:n], x0[int(starts[1]):][:n]])
    a = oc.shape_args(name, 0)
    h = api.Ofdm(n_streams=S, **a)
    M, N = h.n_sym, h.n_fft
    d_in = api.DeviceArray.from_numpy(np.concatenate([x.view(F32).ravel(), np.zeros(64, F32)]))
    d_idx, d_gate = api.DeviceArray.from_numpy(np.zeros(S * nb + 8, F32)), api.DeviceArray.from_numpy(np.ones(S * nb + 8, F32))
    sentinel = np.full(S * nb * M * 2 + 64, SENT, F32)
    d_out, d_ch, d_rec, d_st = (api.DeviceArray.from_numpy(sentinel) for _ in range(4))
    lib = L.load()
    k = C.c_size_t(7)

    def call(pi=d_in.ptr, n_in=n, in_stride=n, px=d_idx.ptr, pg=d_gate.ptr, n_bursts=nb, po=d_out.ptr, ostride=M, pc=d_ch.ptr, pr=d_rec.ptr,
             ps=d_st.ptr, sstride=nb, stream=None, hh=None, base=0, step=2):
        rc = lib.sfe_dsp_ofdm_process_stream(hh or h._h, pi, n_in, in_stride, px, nb, pg, nb, n_bursts, base, step, po, ostride, pc, pr, ps, sstride,
                                             C.byref(k), stream)
        if rc != L.SFE_OK:
            msg = lib.sfe_dsp_last_error()
            assert k.value == 0 and (hh is not None or msg.startswith(b"ofdm_process_stream: ")), msg
        return rc

    assert call(ostride=M - 1) == L.SFE_ERANGE                       # a burst's symbols one short
    assert call(sstride=nb - 1) == L.SFE_ERANGE
    assert call(pi=None) == L.SFE_EINVAL and call(po=None) == L.SFE_EINVAL
    assert call(pi=d_in.ptr + 4) == L.SFE_EINVAL                     # misaligned, each of the seven
    assert call(po=d_out.ptr + 4) == L.SFE_EINVAL
    assert call(pc=d_ch.ptr + 4) == L.SFE_EINVAL
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
    assert call(pc=d_in.ptr) == L.SFE_EINVAL and call(pr=d_in.ptr) == L.SFE_EINVAL and call(ps=d_in.ptr + 16) == L.SFE_EINVAL
    assert call(po=d_idx.ptr) == L.SFE_EINVAL and call(pc=d_idx.ptr) == L.SFE_EINVAL and call(pr=d_idx.ptr + 4) == L.SFE_EINVAL
    assert call(ps=d_idx.ptr + 4 * (S * nb - 1)) == L.SFE_EINVAL
    assert call(po=d_gate.ptr) == L.SFE_EINVAL and call(pc=d_gate.ptr) == L.SFE_EINVAL and call(pr=d_gate.ptr) == L.SFE_EINVAL
    assert call(ps=d_gate.ptr) == L.SFE_EINVAL
    assert call(pr=d_out.ptr + 8) == L.SFE_EINVAL                    # two outputs over one another
    assert call(pc=d_out.ptr + 8 * (S * nb * M - 1)) == L.SFE_EINVAL
    assert call(ps=d_out.ptr + 4 * (S * nb * M * 2 - 1)) == L.SFE_EINVAL
    assert call(ps=d_rec.ptr + 4) == L.SFE_EINVAL and call(pr=d_ch.ptr + 8 * (S * nb * N - 1)) == L.SFE_EINVAL
    assert lib.sfe_dsp_ofdm_process_stream(h._h, d_in.ptr, n, n, None, 0, None, 0, nb, 0, 2, d_out.ptr, M, None, None, None, 0, None, None) == L.SFE_EINVAL
    assert lib.sfe_dsp_last_error().startswith(b"ofdm_process_stream: ")
    assert call(n_bursts=0) == L.SFE_OK and k.value == 0             # no bursts: a no-op
    # a live handle of another block is refused by every ofdm function, and ofdm's destroy frees nothing of it
    other = api.Corr(np.ones(13, np.complex64), 3840)
    assert call(hh=other._h) == L.SFE_EINVAL and k.value == 0
    assert lib.sfe_dsp_ofdm_set_input_format(other._h, L.FMT_U8) == L.SFE_EINVAL and lib.sfe_dsp_ofdm_destroy(other._h) == L.SFE_OK
    other.reset()                                                    # still alive
    other.close()
    assert lib.sfe_dsp_ofdm_set_input_format(h._h, 7) == L.SFE_EINVAL
    with pytest.raises(AttributeError):
        h.reset()
    api.sync()
    for d in (d_out, d_ch, d_rec, d_st):
        assert np.array_equal(_bits(d.to_numpy()), _bits(sentinel))
    # the next good call is a fresh handle's
    assert call() == L.SFE_OK and k.value == nb
    fresh = api.Ofdm(n_streams=S, **a)
    want = fresh.receive(x, idx=np.zeros((S, nb)), gate=np.ones((S, nb)), start_step=2)
    fresh.close()
    assert not want[3].any()
    assert np.array_equal(_bits(d_out.to_numpy(S * nb * M * 2)), _bits(want[0]).ravel())
    assert np.array_equal(_bits(d_ch.to_numpy(S * nb * N * 2)), _bits(want[1]).ravel())
    assert np.array_equal(_bits(d_rec.to_numpy(S * nb * 8)), _bits(want[2]).ravel())
    assert np.array_equal(d_st.to_numpy(S * nb).view(np.int32), want[3].ravel())
    h.close()
    for d in (d_in, d_idx, d_gate, d_out, d_ch, d_rec, d_st):
        d.free()


@pytest.mark.parametrize("name", ["n64", "n4096"])
def test_a_captured_call_replays_to_the_eager_bits(api, L, name):
    """The handle has no setter but the input format, taken by value at enqueue: a call is captured (u8 input, the format
    changed back afterwards), and replayed twice onto poisoned outputs; both times the bits are the eager call's."""
    hip = hip_runtime()
    x0, starts, _ = oc.stream(name)
    x = x0 * (0.7 / np.abs(x0.view(F32)).max())
    by = np.clip(np.rint(x.view(F32).astype(np.float64) * 127.0 + 128.0), 0, 255).astype(np.uint8)
    a = oc.shape_args(name, 1)
    h = api.Ofdm(**a)
    h.set_input_format(L.FMT_U8)
    kw = dict(idx=starts, out_pad=1, st_pad=1, lead=1)
    eager = run(api, h, by, len(starts), **kw)
    assert not eager[3].any()
    sm, g, ex = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert hip.hipStreamCreate(C.byref(sm)) == 0
    r = Run(api, h, by, len(starts), stream=sm.value, launch=False, **kw)
    assert hip.hipStreamBeginCapture(sm, 0) == 0
    try:
        r.launch()
    finally:
        ended = hip.hipStreamEndCapture(sm, C.byref(g))
    assert ended == 0 and r.k == len(starts) and hip.hipGraphInstantiate(C.byref(ex), g, None, None, 0) == 0
    h.set_input_format(L.FMT_F32)                   # the captured call keeps the format it took
    try:
        sent = _bits(np.array([SENT]))[0]
        assert all((_bits(d.to_numpy()) == sent).all() for d in r.d)           # capture ran nothing
        for _ in range(2):
            r.poison()
            assert hip.hipGraphLaunch(ex, sm) == 0 and hip.hipStreamSynchronize(sm) == 0
            assert same(eager, r.read())
    finally:
        hip.hipGraphExecDestroy(ex)
        hip.hipGraphDestroy(g)
        hip.hipStreamDestroy(sm)
        h.close()
        r.free()


def test_the_chain_from_payload_to_payload_stays_on_the_device(api, L):
    """Ldpc.encode_stream's codewords come back to the host once, to be mapped onto the waveform there (the device OFDM
    modulator is not built yet); the waveform is uploaded, and from there on Corr -> Ofdm (MRC) -> Ldpc.process_stream pass
    handles, pointers and strides only.  The host plans say first where the peaks must stand."""
    c = oc.CHAIN
    x, pay, (pval, pidx), pdec, prec = oc.chain_on_the_cpu(api, L, lc)
    s, Z = lc.CASES["B"]
    a_, beta, max_iter = lc.PARAMS["a12"]
    enc = api.Ldpc(s, Z, lc.SCALE, a_, beta, max_iter, in_mode=L.VIT_IN_QPSK, skip=0)
    code = np.unpackbits(enc.encode(pay), axis=1)[:, :648]
    assert np.array_equal(oc.chain_signal(code), x)                 # the device's codewords are the plan's
    nblk, B = c["n_blocks"], c["block"]
    corr = api.Corr(oc.chain_template(), B)
    rx = api.Ofdm(**oc.shape_args("n64", 1, c["min_gate"]))
    M = rx.n_sym
    assert M == 324 and enc.row == 324
    d_x = api.DeviceArray.from_numpy(x.view(F32))
    d_val, d_idx = api.DeviceArray(nblk), api.DeviceArray(nblk)
    nb = 3                                                           # blocks 1, 2 and 3 hold the bursts
    d_sym, d_rec, d_st = api.DeviceArray(nb * M * 2), api.DeviceArray(nb * 8), api.DeviceArray(nb)
    d_bits, d_lrec, d_lst = api.DeviceArray(nb * 11), api.DeviceArray(nb * 3), api.DeviceArray(nb)
    held = (d_x, d_val, d_idx, d_sym, d_rec, d_st, d_bits, d_lrec, d_lst)
    try:
        assert corr.process_stream(d_x, x.size, d_val, d_idx) == nblk
        assert rx.process_stream(d_x, x.size, nb, d_sym, d_idx.ptr + 4, d_val.ptr + 4, None, d_rec, d_st, start_base=B - 79, start_step=B) == nb
        assert enc.process_stream(d_sym, nb, d_bits, d_lrec, d_lst, d_status_in=d_st, in_stride=M, out_stride=44) == nb
        api.sync()
        idx, val = d_idx.to_numpy().view(np.uint32), d_val.to_numpy()
        st, lst = d_st.to_numpy().view(np.int32), d_lst.to_numpy().view(np.int32)
        by = d_bits.to_numpy().view(np.uint8).reshape(nb, 44)[:, :41]
        lrec = d_lrec.to_numpy().view(np.uint32).reshape(nb, 3)
        rec = d_rec.to_numpy().reshape(nb, 8)
    finally:
        for d in held:
            d.free()
        for q in (corr, rx, enc):
            q.close()
    print("peaks", val, idx, "receiver", st, "eps", rec[:, 0], "decoder", lst, "iterations", lrec[:, 0], "repairs", lrec[:, 2])
    assert idx[[1, 2, 3]].tolist() == pidx[[1, 2, 3]].tolist()      # the peaks first: a wrong one is the correlator's, not the receiver's
    assert (val[[1, 2, 3]] >= c["min_gate"]).all()
    assert not st.any() and not lst.any()                           # every status is 0
    assert np.array_equal(by, lc.payload_bits_only("B", pay))
    assert lrec[:, 2].max() >= 1 and not lrec[:, 1].any()           # wrong hard decisions went in, none came out
    assert (np.abs(rec.astype(np.float64) - prec) <= 1e-5 + 1e-4 * np.abs(prec.astype(np.float64))).all()       # the receiver's record: the plan's
