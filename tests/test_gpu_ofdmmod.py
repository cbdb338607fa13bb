"""The OFDM burst modulator (sfe_dsp_ofdmmod_*) on the GPU.  The bar is equality with api.ofdmmod_plan -- float32 words or
wire-format bytes -- never a tolerance.  Every output sits between guards and is poisoned before every call (the poison and
guard idea of tests/stream_checks.py): after the call no poison is left in the stream's n_out samples, the guards are
intact, and every sample in no frame is +0.  Every instantiation, the contracts about bits, a captured call, the
refusals, a relay behind the receiver, and the loop Ldpc.encode_stream -> OfdmMod -> Corr -> Ofdm -> Ldpc.process_stream
on the device."""
import ctypes as C

import numpy as np
import pytest

import ldpc_cases as lc
import mod_checks as mchk
import ofdm_cases as oc
import ofdmmod_cases as mc
import stream_checks as sc
from simplefe_amd import synth

pytestmark = pytest.mark.gpu
F32 = np.float32
GUARD = 64                          # bytes before and behind the output
same = mc.same


@pytest.fixture(scope="module")
def api():
    from simplefe_amd import api as a
    return a


@pytest.fixture(scope="module")
def L():
    from simplefe_amd import lib
    return lib


class Out:
    """A poisoned, guarded output on the device: the stream's bytes start `shift` bytes behind an aligned front guard."""

    def __init__(self, api, n_out, tx10, shift=0):
        self.api, self.nbytes, self.front = api, (n_out // 2 * 5 if tx10 else 8 * n_out), GUARD + shift
        self.words = (self.front + self.nbytes + GUARD + 3) // 4
        self.d = api.DeviceArray(self.words)
        self.ptr = self.d.ptr + self.front
        self.tx10 = tx10
        self.poison()

    def poison(self):
        raw = np.full(self.words, sc.POISON, np.uint32)
        self.api.check(self.d._L.sfe_dsp_memcpy_h2d(self.d.ptr, raw.ctypes.data, raw.nbytes, None))
        self.api.sync()

    def take(self):
        """The stream's bytes, after checking that none of its cells kept the poison and that the guards did."""
        raw = self.d.to_numpy().view(np.uint8)
        kept_poison = raw == np.full(self.words, sc.POISON, np.uint32).view(np.uint8)
        assert kept_poison[:self.front].all() and kept_poison[self.front + self.nbytes:].all(), "a store outside the stream"
        cell = 5 if self.tx10 else 4
        body = kept_poison[self.front:self.front + self.nbytes]
        kept = np.array([body[i::cell][:self.nbytes // cell] for i in range(cell)]).all(axis=0)
        assert not kept.any(), "%d cells of the stream were never stored, the first at %d" % (int(kept.sum()), int(np.flatnonzero(kept)[0]))
        got = raw[self.front:self.front + self.nbytes].copy()
        return got if self.tx10 else got.view(np.complex64)

    def free(self):
        self.d.free()


def run(api, h, data, n_out, start_base=0, start_step=0, in_pad=0, lead=0, shift=0):
    """One call: burst b's row `lead` elements into a guarded input buffer and in_pad elements behind the row before it;
    returns the stream."""
    symbols = h.in_mode == mc.SYMBOLS
    data = np.ascontiguousarray(np.atleast_2d(data), np.complex64 if symbols else np.uint8)
    nb, stride = data.shape[0], data.shape[1] + in_pad
    buf = np.full(lead + nb * stride + 3, 0.25 + 0.5j if symbols else 0x5A, data.dtype)
    for b in range(nb):
        buf[lead + b * stride:][:data.shape[1]] = data[b]
    d_in = sc.from_numpy(api, buf.view(F32)) if symbols else sc.from_bytes(api, buf)
    out = Out(api, n_out, h.out_fmt == mc.TX10, shift)
    try:
        k = h.process_stream(d_in.ptr + lead * data.itemsize, nb, out.ptr, n_out, start_base, start_step, in_stride=stride)
        api.sync()
        assert k == n_out
        return out.take()
    finally:
        d_in.free()                 # the guards of the input and its contents are checked here
        out.free()


def zeros_outside(got, starts, F, tx10):
    """Every sample of the stream in no frame: the bit pattern of +0, or under TX10 the group of two zeros."""
    n = got.size // 5 * 2 if tx10 else got.size
    inside = np.zeros(n, bool)
    for o in starts:
        inside[o:o + F] = True
    if tx10:
        g = got.reshape(-1, 5)[~inside[0::2]]
        return bool((g == [0xAA, 0, 0, 0, 0]).all())
    return not got[~inside].view(np.uint32).any()


# ---- every instantiation
@pytest.mark.parametrize("fmt", ["f32", "tx10"])
@pytest.mark.parametrize("name", oc.GRID_NAMES)
def test_every_instantiation_equals_the_plan(api, L, name, fmt):
    """log2 N = 6 .. 12 with every bin used, with and without pilots, Nd = 1 among them; BITS order 2 and 4, and SYMBOLS; three
    bursts and one.  F32: an odd start_base and an odd cp -- the shape's own where it is odd, else 1 more, and 3, smaller than a
    wave -- cp = N and cp = 0, at both 16-byte phases of the output's address.  TX10: even values, any byte address."""
    sh = oc.shape(name)
    N = sh["n_fft"]
    cps = sorted({sh["cp"] | 1, 3, N, 0}) if fmt == "f32" else sorted({sh["cp"] + (sh["cp"] & 1), 2, N})
    out_fmt = L.FMT_TX10 if fmt == "tx10" else L.FMT_F32
    n_data = min(sh["n_data"], 2)
    for ci, cp in enumerate(cps):
        for mid, order, in_mode in mc.MODES if ci == 0 else mc.MODES[1 + ci % 2:][:1]:
            args = mc.shape_args(name, amp=0.5, order=order, in_mode=in_mode, out_fmt=out_fmt, cp=cp, n_data=n_data)
            F = mc.sizes(args)[3]
            h = api.OfdmMod(**args)
            assert (h.frame_len, h.n_in, h.n_sym) == (F, mc.sizes(args)[4], n_data * mc.sizes(args)[0])
            data = mc.rows(args, 3, 7 + ci)
            odd = 0 if fmt == "tx10" else 1
            for nb, base, step, tail in ((3, 4 + odd, F + 6 + odd, 2 + odd), (1, 0, 0, 0), (3, 0, F, 0)):
                place = dict(n_out=base + (nb - 1) * step + F + tail, start_base=base, start_step=step)
                want = api.ofdmmod_plan(**args, data=data[:nb], **place)
                got = run(api, h, data[:nb], in_pad=2, lead=1, shift=(8 * (ci & 1)) if fmt == "f32" else 3, **place)
                assert same(got, want), (name, fmt, cp, mid, nb, base)
                assert zeros_outside(got, base + np.arange(nb) * step, F, fmt == "tx10"), (name, fmt, cp, mid, nb)
            h.close()


def test_gaps_longer_than_a_zero_tile(api, L):
    """A lead-in, gaps and a tail of more than one tile of zeros each, none a multiple of it, F32 and TX10."""
    _, zt, _ = api.ofdmmod_footprint(256)
    for out_fmt in (L.FMT_F32, L.FMT_TX10):
        args = mc.shape_args("g256", amp=0.5, out_fmt=out_fmt, cp=8, n_data=1)
        F = mc.sizes(args)[3]
        h = api.OfdmMod(**args)
        data = mc.rows(args, 3, 2)
        base, step = zt + 10, F + 2 * zt + 6
        place = dict(n_out=base + 2 * step + F + zt + 18, start_base=base, start_step=step)
        got = run(api, h, data, shift=8, **place)
        assert same(got, api.ofdmmod_plan(**args, data=data, **place))
        assert zeros_outside(got, base + np.arange(3) * step, F, out_fmt == L.FMT_TX10)
        h.close()


def test_no_bursts_write_zeros(api, L):
    for out_fmt, shift in ((L.FMT_F32, 8), (L.FMT_TX10, 3)):
        args = mc.shape_args("g64", out_fmt=out_fmt)
        h = api.OfdmMod(**args)
        got = run(api, h, np.zeros((0, 1), np.uint8), 9000, shift=shift)
        assert same(got, api.ofdmmod_plan(**args, data=np.zeros((0, 1), np.uint8), n_out=9000))
        assert not got.view(np.uint8).any() if out_fmt == L.FMT_F32 else (got.reshape(-1, 5) == [0xAA, 0, 0, 0, 0]).all()
        h.close()


# ---- the contracts about bits
@pytest.mark.parametrize("fmt", ["f32", "tx10"])
@pytest.mark.parametrize("mode", mc.MODES[1:], ids=mc.MODE_IDS[1:])
def test_runs_repeat_and_a_frame_depends_on_its_row_alone(api, L, mode, fmt):
    """The same call twice; a 3-burst call against three 1-burst calls at other addresses, strides and offsets; the prefix of
    every symbol is its tail, bit for bit."""
    _, order, in_mode = mode
    tx10 = fmt == "tx10"
    args = mc.shape_args("g1024", amp=0.5, order=order, in_mode=in_mode, out_fmt=L.FMT_TX10 if tx10 else L.FMT_F32, n_data=2)
    Nd, nsym, Ls, F, n = mc.sizes(args)
    h = api.OfdmMod(**args)
    data = mc.rows(args, 3, 31)
    place = dict(n_out=3 * (F + 6) + 10, start_base=4, start_step=F + 6)
    a = run(api, h, data, in_pad=3, lead=2, shift=8, **place)
    b = run(api, h, data, in_pad=3, lead=2, shift=8, **place)
    assert same(a, b) and same(a, api.ofdmmod_plan(**args, data=data, **place))
    for i in range(3):
        base = 2 * i + 6 + (0 if tx10 else 1)
        one = run(api, h, data[i], in_pad=i, lead=1 + i, shift=(i % 2) * 8 if not tx10 else i, n_out=base + F + 6 + base % 2, start_base=base)
        if tx10:
            assert np.array_equal(one[base // 2 * 5:][:F // 2 * 5], a[(4 + i * (F + 6)) // 2 * 5:][:F // 2 * 5]), i
        else:
            assert same(one[base:base + F], a[4 + i * (F + 6):][:F]), i
    if not tx10:
        y = a[4:4 + F].reshape(nsym, Ls)
        assert same(np.ascontiguousarray(y[:, :args["cp"]]), np.ascontiguousarray(y[:, 1024:1024 + args["cp"]]))
    h.close()


@pytest.mark.parametrize("name", ["g64", "g2048", "n512"])
def test_the_exact_case_on_the_device(api, L, name):
    args = mc.exact_args(name)
    Nd, nsym, Ls, F, n = mc.sizes(args)
    h = api.OfdmMod(**args)
    y = run(api, h, np.zeros((1, n), np.uint8), F + 3, start_base=3, shift=8)
    h.close()
    want = np.zeros((nsym, Ls), np.complex64)
    want[:, args["cp"]] = 1.0
    if args["cp"] == args["n_fft"]:
        want[:, 0] = 1.0                                         # the prefix is the whole symbol
    assert (y[3:].reshape(nsym, Ls) == want).all() and not y[:3].view(np.uint32).any()


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


def test_a_captured_call_replays_onto_a_poisoned_output(api, L):
    """Nothing in a handle changes after create, so a call under graph capture is supported: the node is replayed twice,
    the output poisoned again in between, and both times the stream equals the plan's."""
    hip = hip_runtime()
    args = mc.shape_args("n64", amp=0.5)
    F = mc.sizes(args)[3]
    h = api.OfdmMod(**args)
    data = mc.rows(args, 3, 9)
    place = dict(n_out=3 * F + 40, start_base=11, start_step=F + 7)
    want = api.ofdmmod_plan(**args, data=data, **place)
    d_in, out = api.DeviceArray.from_bytes(data), Out(api, place["n_out"], False, 8)
    s, g, ex = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert hip.hipStreamCreate(C.byref(s)) == 0
    assert hip.hipStreamBeginCapture(s, 0) == 0
    try:
        k = h.process_stream(d_in, 3, out.ptr, place["n_out"], place["start_base"], place["start_step"], stream=s.value)
    finally:
        ended = hip.hipStreamEndCapture(s, C.byref(g))
    assert ended == 0 and k == place["n_out"] and hip.hipGraphInstantiate(C.byref(ex), g, None, None, 0) == 0
    try:
        for _ in range(2):
            out.poison()
            assert hip.hipGraphLaunch(ex, s) == 0 and hip.hipStreamSynchronize(s) == 0
            assert same(out.take(), want)
    finally:
        hip.hipGraphExecDestroy(ex)
        hip.hipGraphDestroy(g)
        hip.hipStreamDestroy(s)
        h.close()
        d_in.free()
        out.free()


def test_refusals_launch_nothing(api, L):
    args = mc.shape_args("n64", amp=0.5)
    h = api.OfdmMod(**args)
    ht = api.OfdmMod(**{**args, "out_fmt": L.FMT_TX10})
    hs = api.OfdmMod(**{**args, "in_mode": L.OFDMMOD_IN_SYMBOLS})
    F, nbytes, nb = h.frame_len, h.n_bytes, 3
    assert (h.n_data_bins, h.n_sym, F, nbytes, h.n_in, hs.n_in) == (54, 324, 640, 81, 81, 324)
    data = mc.rows(args, nb, 41)
    n_out = nb * F + 6
    d_in = api.DeviceArray.from_bytes(np.concatenate([data.ravel(), np.zeros(64, np.uint8)]))
    d_sym = api.DeviceArray(2 * nb * 324 + 4)
    out = Out(api, n_out, False, 0)
    lib = L.load()
    k = C.c_size_t(7)

    def call(pi=d_in.ptr, istride=nbytes, n_bursts=nb, base=2, step=F, po=out.ptr, n=n_out, hh=h._h, kk=C.byref(k)):
        return lib.sfe_dsp_ofdmmod_process_stream(hh, pi, istride, n_bursts, base, step, po, n, kk, None)

    assert call(istride=nbytes - 1) == L.SFE_ERANGE and lib.sfe_dsp_last_error().startswith(b"ofdmmod_process_stream: ")
    assert call(hh=hs._h, pi=d_sym.ptr, istride=323) == L.SFE_ERANGE                 # a short stride in cf32
    assert call(pi=None) == L.SFE_EINVAL and call(po=None) == L.SFE_EINVAL
    assert call(po=out.ptr + 4) == L.SFE_EINVAL                      # cf32 output is eight-byte aligned
    assert call(hh=hs._h, pi=d_sym.ptr + 4, istride=324) == L.SFE_EINVAL             # and so are cf32 symbols
    assert call(base=-1) == L.SFE_EINVAL and call(step=F - 1) == L.SFE_EINVAL
    assert call(base=7) == L.SFE_EINVAL and call(n=n_out - 5) == L.SFE_EINVAL     # the last frame would end behind the stream
    assert call(n=1 << 31) == L.SFE_EINVAL and call(n_bursts=1 << 31) == L.SFE_EINVAL
    assert call(hh=ht._h, n=n_out - 1) == L.SFE_EINVAL               # an odd n_out under TX10
    assert call(hh=ht._h, base=3) == L.SFE_EINVAL and call(hh=ht._h, base=0, step=F + 1) == L.SFE_EINVAL     # odd placement under TX10
    assert lib.sfe_dsp_last_error().startswith(b"ofdmmod_process_stream: ")
    assert call(n_bursts=2, istride=1 << 62) == L.SFE_EINVAL         # a byte range that reaches 2^62
    assert call(po=d_in.ptr + 8 * ((nb * nbytes - 1) // 8)) == L.SFE_EINVAL      # the output over the input
    assert call(pi=out.ptr + 8 * n_out - 1) == L.SFE_EINVAL
    assert call(kk=None) == L.SFE_EINVAL and call(hh=None) == L.SFE_EINVAL
    assert k.value == 0
    # a live handle of another block is refused, and ofdmmod's destroy frees nothing of it; a destroyed handle is refused
    other = api.Corr(np.ones(13, np.complex64), 3840)
    assert call(hh=other._h) == L.SFE_EINVAL and k.value == 0
    assert lib.sfe_dsp_last_error().startswith(b"not a live") or lib.sfe_dsp_last_error().startswith(b"ofdmmod_process_stream: ")
    assert lib.sfe_dsp_ofdmmod_destroy(other._h) == L.SFE_OK
    other.reset()                                                    # still alive
    other.close()
    with pytest.raises(AttributeError):
        h.reset()
    api.sync()
    raw = out.d.to_numpy().view(np.uint32)
    assert (raw == sc.POISON).all()
    # the next good call is a fresh handle's; TX10 output and the coded bytes need no alignment
    assert call() == L.SFE_OK and k.value == n_out
    api.sync()
    assert same(out.take(), api.ofdmmod_plan(**args, data=data, n_out=n_out, start_base=2, start_step=F))
    out.poison()
    assert call(n_bursts=0, pi=None) == L.SFE_OK and k.value == n_out
    api.sync()
    assert not out.take().view(np.uint8).any()
    assert call(n=0, n_bursts=0, po=None, pi=None) == L.SFE_OK and k.value == 0
    outt = Out(api, n_out, True, 3)
    assert call(hh=ht._h, pi=d_in.ptr + 1, istride=nbytes + 1, n_bursts=2, po=outt.ptr) == L.SFE_OK
    api.sync()
    shifted = np.concatenate([data.ravel(), np.zeros(64, np.uint8)])[1:][:2 * (nbytes + 1)].reshape(2, nbytes + 1)
    assert same(outt.take(), api.ofdmmod_plan(**{**args, "out_fmt": L.FMT_TX10}, data=shifted, n_out=n_out, start_base=2, start_step=F))
    assert same(h.modulate(data, n_out, 2, F), api.ofdmmod_plan(**args, data=data, n_out=n_out, start_base=2, start_step=F))
    for x in (h, ht, hs):
        x.close()
    out.poison()
    with pytest.raises(api.SfeError) as e:                           # a use after destroy: the wrapper holds no handle any more
        h.process_stream(d_in, nb, out.ptr, n_out, 2, F)
    assert e.value.code == L.SFE_EINVAL
    api.sync()
    assert (out.d.to_numpy().view(np.uint32) == sc.POISON).all()
    for d in (d_in, d_sym, out, outt):
        d.free()


# ---- behind the receiver, and around the loop
def test_a_relay_reads_the_receivers_rows_as_they_lie(api, L):
    """An Ofdm handle's d_out and out_stride go straight into an OfdmMod in SYMBOLS mode (a non-regenerative relay): the
    stream equals the plan's on the received symbols."""
    name, nb = "n64", 3
    x, starts, _ = oc.stream(name, nb)
    rx = api.Ofdm(**oc.shape_args(name))
    args = mc.shape_args(name, amp=0.5, in_mode=mc.SYMBOLS)
    tx = api.OfdmMod(**args)
    M, F, ostride = rx.n_sym, tx.frame_len, rx.n_sym + 5
    assert tx.n_in == M
    n_out = nb * (F + 1) + 9
    d_x, d_idx = api.DeviceArray.from_numpy(np.asarray(x).view(F32)), api.DeviceArray.from_numpy(starts.astype(np.uint32).view(F32))
    d_sym, d_st = sc.device_array(api, 2 * nb * ostride), api.DeviceArray(nb)
    out = Out(api, n_out, False, 8)
    try:
        assert rx.process_stream(d_x, x.size, nb, d_sym, d_idx, d_status=d_st, out_stride=ostride) == nb
        assert tx.process_stream(d_sym.ptr, nb, out.ptr, n_out, 3, F + 1, in_stride=ostride) == n_out
        api.sync()
        got = out.take()
        assert not d_st.to_numpy().view(np.int32).any()
        rows = d_sym.to_numpy(keep=True).view(np.complex64).reshape(nb, ostride)[:, :M]
    finally:
        for d in (d_x, d_idx, d_sym, d_st, out):
            d.free()
        rx.close()
        tx.close()
    assert same(got, api.ofdmmod_plan(**args, data=np.ascontiguousarray(rows), n_out=n_out, start_base=3, start_step=F + 1))


# The loop's three frames stand where oc.CHAIN puts them; a call lays its frames at one spacing, so each frame is a call of its
# own on its part of the stream.  Under TX10 a part starts on an even sample of its own numbering and frame 2 stands at an odd
# sample of the stream, so its part starts one sample late: the three parts are streams of their own, laid into the (I,Q)
# byte stream on the host, where the wire format is re-read as the receive format anyway; the two samples between the parts
# are zeros there.
# The correlator's template is the modulator's own stream from TPL_LEAD samples before a frame to the end of its first training
# symbol, prefix included.  The two training symbols of a frame are the same words, so on this noiseless stream a template of
# the symbol alone has two EQUAL peaks 80 samples apart and rounding would choose between them; with the lead-in's zeros in
# the template the window of the second peak holds TPL_LEAD samples of the first symbol more, and its value falls to about 0.8.
TPL_LEAD = 16
PARTS = {False: ((0, 7680), (7680, 11520), (11520, 19200)), True: ((0, 7680), (7681, 11519), (11520, 19200))}


def loop_amp(api, L, code):
    """The largest power of two at which no component of the three frames reaches 1.0 (the wire format wraps there), by the plan."""
    args = mc.shape_args("n64", amp=1.0)
    F = mc.sizes(args)[3]
    peak = max(float(np.abs(api.ofdmmod_plan(**args, data=row, n_out=F).view(F32)).max()) for row in code)
    return float(2.0 ** np.floor(np.log2(0.99 / peak)))


def loop_on_the_cpu(api, L, tx10):
    """The loop through the host plans: (payloads, amp, the template, the plan's stream as the receiver reads it).  Asserts
    that the F32 peak is below 1.0 and that the plan-side chain decodes every payload with every status 0."""
    c = oc.CHAIN
    s, Z = lc.CASES["B"]
    a_, beta, max_iter = lc.PARAMS["a12"]
    pay = lc.payloads("B", 3, 77)
    code = api.ldpc_plan(s, Z, data=pay)
    assert code.shape == (3, 81)
    amp = loop_amp(api, L, code)
    args = mc.shape_args("n64", amp=amp)
    F, n = mc.sizes(args)[3], c["n_blocks"] * c["block"]
    x = np.zeros(n, np.complex64)
    for row, o in zip(code, c["at"].values()):
        x[o:o + F] = api.ofdmmod_plan(**args, data=row, n_out=F)
    assert float(np.abs(x.view(F32)).max()) < 1.0
    tpl = x[c["at"][1] - TPL_LEAD:][:TPL_LEAD + 80].copy()           # the modulator's own first training symbol behind its lead-in
    if tx10:
        u8 = mchk.tx10_as_u8_samples(synth.tx10_pack(x))
        x = ((u8.astype(F32) - F32(128.0)) * F32(1.0 / 127.0)).view(np.complex64)
    m, val, idx = synth.corr_reference(x, tpl[None, :], c["block"], 0.0)
    for j, o in c["at"].items():
        assert idx[0, j] == o - j * c["block"] + 79 and val[0, j] >= 1.2 * c["min_gate"], (j, idx[0, j], val[0, j])
        assert m[0, o + 79] >= 1.1 * m[0, o + 159], (j, m[0, o + 79], m[0, o + 159])        # the second training symbol's peak stands clearly lower
    sym, ch, rec, st = api.ofdm_plan(x=x, idx=idx[0, 1:4].astype(np.uint32), gate=val[0, 1:4].astype(F32), start_base=c["block"] - 79,
                                     start_step=c["block"], **oc.shape_args("n64", 1, c["min_gate"]))
    assert not st.any()
    dec = api.ldpc_plan(s, Z, lc.SCALE, a_, beta, max_iter, in_mode=L.VIT_IN_QPSK, skip=0, x=sym.reshape(3, -1), status_in=st)
    assert not dec[2].any() and np.array_equal(dec[0], lc.payload_bits_only("B", pay))
    return pay, amp, tpl, idx[0]


@pytest.mark.parametrize("fmt", ["f32", "tx10-as-u8"])
def test_the_loop_from_payload_to_payload_on_the_device(api, L, fmt):
    """Ldpc.encode_stream -> OfdmMod -> Corr -> Ofdm (MRC) -> Ldpc.process_stream on the n64 shape and code B, three codewords at
    oc.CHAIN's offsets, the correlator's template the modulator's own first training symbol behind its lead-in (TPL_LEAD).  In F32 nothing comes to the host
    between the blocks.  With TX10 the receive side reads a host-side requantisation of the wire format to (I,Q) bytes: there
    is no TX10 -> u8 converter on the device.  Every status is 0, every payload comes back, and the F32 waveform is the
    float64 synthesiser's within 1e-5 relative RMS per symbol."""
    c = oc.CHAIN
    u8 = fmt != "f32"
    pay, amp, tpl, pidx = loop_on_the_cpu(api, L, u8)
    s, Z = lc.CASES["B"]
    a_, beta, max_iter = lc.PARAMS["a12"]
    ldpc = api.Ldpc(s, Z, lc.SCALE, a_, beta, max_iter, in_mode=L.VIT_IN_QPSK, skip=0)
    args = mc.shape_args("n64", amp=amp, out_fmt=L.FMT_TX10 if u8 else L.FMT_F32)
    tx = api.OfdmMod(**args)
    corr = api.Corr(tpl, c["block"])
    rx = api.Ofdm(**oc.shape_args("n64", 1, c["min_gate"]))
    if u8:
        corr.set_input_format(L.FMT_U8)
        rx.set_input_format(L.FMT_U8)
    nblk, B, F, M, nb = c["n_blocks"], c["block"], tx.frame_len, rx.n_sym, 3
    n = nblk * B
    assert (tx.n_in, ldpc.n_bytes, M, ldpc.row) == (81, 81, 324, 324)
    cstride = 84                                                     # the codewords' rows, a few bytes apart
    d_pay, d_code = api.DeviceArray.from_bytes(pay), sc.device_array(api, nb * cstride // 4)       # the encoder's output, poisoned and guarded
    outs = [Out(api, hi - lo, u8, 0) for lo, hi in PARTS[u8]] if u8 else [Out(api, n, False, 0)]
    d_val, d_idx = api.DeviceArray(nblk), api.DeviceArray(nblk)
    d_sym, d_rec, d_st = api.DeviceArray(nb * M * 2), api.DeviceArray(nb * 8), api.DeviceArray(nb)
    d_bits, d_lrec, d_lst = api.DeviceArray(nb * 11), api.DeviceArray(nb * 3), api.DeviceArray(nb)
    held = [d_pay, d_code, d_val, d_idx, d_sym, d_rec, d_st, d_bits, d_lrec, d_lst] + outs
    try:
        assert ldpc.encode_stream(d_pay, nb, d_code.ptr, out_stride=cstride) == nb
        for b, ((lo, hi), o) in enumerate(zip(PARTS[u8], c["at"].values())):
            po = outs[b].ptr if u8 else outs[0].ptr + 8 * lo
            assert tx.process_stream(d_code.ptr + b * cstride, 1, po, hi - lo, o - lo) == hi - lo
        x = outs[0].ptr
        if u8:
            api.sync()
            wire = np.full(2 * n, 128, np.uint8)
            for (lo, hi), o in zip(PARTS[u8], outs):
                wire[2 * lo:2 * hi] = mchk.tx10_as_u8_samples(o.take())
            held.append(api.DeviceArray.from_bytes(wire))
            x = held[-1].ptr
        assert corr.process_stream(x, n, d_val, d_idx) == nblk
        assert rx.process_stream(x, n, nb, d_sym, d_idx.ptr + 4, d_val.ptr + 4, None, d_rec, d_st, start_base=B - 79, start_step=B) == nb
        assert ldpc.process_stream(d_sym, nb, d_bits, d_lrec, d_lst, d_status_in=d_st, in_stride=M, out_stride=44) == nb
        api.sync()
        wave = None if u8 else outs[0].take()
        idx, val = d_idx.to_numpy().view(np.uint32), d_val.to_numpy()
        st, lst = d_st.to_numpy().view(np.int32), d_lst.to_numpy().view(np.int32)
        by = d_bits.to_numpy().view(np.uint8).reshape(nb, 44)[:, :41]
        code = d_code.to_numpy(keep=True).view(np.uint8)[:nb * cstride].reshape(nb, cstride)[:, :81]
    finally:
        for d in held:
            d.free()
        for q in (ldpc, tx, corr, rx):
            q.close()
    print(fmt, "amp", amp, "peaks", val, idx, "receiver", st, "decoder", lst)
    assert idx[[1, 2, 3]].tolist() == pidx[[1, 2, 3]].tolist() and (val[[1, 2, 3]] >= c["min_gate"]).all()
    assert not st.any() and not lst.any()
    assert np.array_equal(by, lc.payload_bits_only("B", pay))
    if not u8:
        want = np.zeros(n, np.complex64)
        worst = 0.0
        for row, o in zip(code, c["at"].values()):
            want[o:o + F] = api.ofdmmod_plan(**args, data=row, n_out=F)
            worst = max(worst, mc.worst_symbol_rms(wave[o:o + F], mc.reference_frame(args, row), args))
        print("the device's noiseless waveform against synth.ofdm_signal: worst symbol rel-RMS %.3e" % worst)
        assert same(wave, want) and worst <= mc.RMS_BAR
