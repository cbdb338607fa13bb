"""The FM, phase and envelope detector on the GPU (sfe_dsp_polar_*, csrc/polar.hip).  The bar is equality with the host plan
(api.polar_plan, the same law compiled for the host; tests/test_polar_host.py holds the plan to the law and to float64) --
float32 words, never a tolerance.  Every call reads from an input that sits at an offset inside a buffer of poison and
writes into an output that is poisoned before the call and sits between guards, rows at odd strides (the layouts and
verdicts of tests/stream_checks.py): exactly the call's n_in cells per row lose their poison, nothing else changes.
`-m gpu`."""
import ctypes as C
import os

import numpy as np
import pytest

import stream_checks as sc
from simplefe_amd import synth

pytestmark = pytest.mark.gpu
FM, PM, AM = synth.POLAR_FM, synth.POLAR_PM, synth.POLAR_AM
SIZES = [1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 4099, 65539]     # head and tail peel, a wave's edge, a workgroup's run, tiles
GAIN = 0.7


@pytest.fixture(scope="module")
def api():
    from simplefe_amd import api as a
    return a


@pytest.fixture(scope="module")
def L():
    from simplefe_amd import lib
    return lib


@pytest.fixture(autouse=True)
def _guards():
    yield
    sc.check_guarded()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want, what):
    got, want = _bits(got), _bits(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    d = got != want
    assert not d.any(), "%s: %d of %d words differ, the first at %s" % (what, int(d.sum()), d.size, np.argwhere(d)[0])


# the exact-value table of tests/test_polar_host.py as samples x + jy, and the denormal pair
TABLE = np.array([0 + 0j, 1 + 0j, 0 + 1j, 0 - 1j, -1 + 0j, 1 + 1j, complex(-1, -0.0), complex(1, -0.0), complex(-0.0, 0), -1 - 1j,
                  complex(np.float32(1e-39), np.float32(1e-40)), complex(np.float32(-1e-40), np.float32(1e-39)), 3 + 4j], np.complex64)


def _streams(n, n_streams, first=0, table=True):
    x = np.stack([synth.synth_cf32(n, ch=20 + s, first_sample=first).view(np.complex64) for s in range(n_streams)])
    if table and n > 2 * TABLE.size:
        x[0, 5:5 + TABLE.size] = TABLE
        x[-1, n - TABLE.size:] = TABLE[::-1]
    return x


def _bytes(n, n_streams, seed=0):
    b = np.stack([synth.offset_bytes(n, seed=seed + 31 * s + 1) for s in range(n_streams)])
    if n >= 8:
        b[0, 4:12] = [128, 128, 0, 255, 255, 0, 128, 127]         # a zero sample, the corners
    return b


def _plan(api, x, mode, in_u8, gain=GAIN):
    """The host plan of every stream, each from a fresh start: (n_streams, n) float32."""
    rows = np.ascontiguousarray(x).reshape(x.shape[0], -1)
    return np.stack([api.polar_plan(r, mode, gain, in_u8=in_u8)[0] for r in rows])


def run_polar(api, h, x, cuts=None, in_u8=False, aligned=True, out_shift=0):
    """Polar.process_stream through poisoned, guarded buffers: x (n_streams, n) complex64 -- (n_streams, 2n) uint8 with
    in_u8 -- fed in calls of the sizes `cuts` (None: one call).  aligned: every row of both buffers starts on a 16-byte
    boundary, at strides that are odd multiples of 16 bytes; else the input starts one sample past such a boundary and
    both strides are odd counts of items, so that the rows' alignments differ.  out_shift: floats between the output's
    first row and a 16-byte boundary.  Returns (n_streams, n) float32."""
    S = h.n_streams
    x = np.ascontiguousarray(x, dtype=np.uint8 if in_u8 else np.complex64).reshape(S, -1)
    item = 2 if in_u8 else 8
    rows = x.view(np.uint8)
    n = rows.shape[1] // item
    pos, outs = 0, []
    for m in cuts or [n]:
        si, so = sc.measure_strides(m, item, m, 4, aligned)
        ilay = sc.Layout(S, item, m, si, 64 + (0 if aligned else item), 64)
        olay = sc.Layout(S, 4, m, so, 256 + 4 * out_shift, 256)
        iraw = ilay.poisoned()
        for s in range(S):
            ilay.put(iraw, s, rows[s, pos * item:(pos + m) * item])
        d_in, d_out = api.DeviceArray.from_numpy(iraw.view(np.float32)), api.DeviceArray.from_numpy(olay.poisoned().view(np.float32))
        try:
            assert d_in.ptr % 16 == 0 and d_out.ptr % 16 == 0
            k = h.process_stream(d_in.ptr + ilay.front, m, d_out.ptr + olay.front, in_stride=si, out_stride=so)
            oraw, iafter = d_out.to_numpy().view(np.uint32), d_in.to_numpy().view(np.uint32)
        finally:
            d_in.free()
            d_out.free()
        if k != m:
            raise sc.CountError("call of %d samples: n_out %d" % (m, k))
        sc.check_written(oraw, olay, m)
        sc.check_input_intact(iafter, iraw)
        outs.append(np.stack([olay.take(oraw, s, m) for s in range(S)]))
        pos += m
    assert pos == n
    return np.concatenate(outs, axis=1)


# ------------------------------------------------------------------------------------------------ the plan's bits
@pytest.mark.parametrize("n_streams", [1, 3])
@pytest.mark.parametrize("in_u8", [False, True], ids=["cf32", "u8"])
@pytest.mark.parametrize("mode", [FM, PM, AM], ids=["fm", "pm", "am"])
def test_the_device_gives_the_plans_bits(api, L, mode, in_u8, n_streams):
    for j, n in enumerate(SIZES):
        x = _bytes(n, n_streams, seed=n) if in_u8 else _streams(n, n_streams)
        want = _plan(api, x, mode, in_u8)
        for aligned in (True, False):
            shift = (j + (0 if aligned else 2)) % 4
            h = api.Polar(mode, GAIN, n_streams=n_streams)
            if in_u8:
                h.set_input_format(L.FMT_U8)
            got = run_polar(api, h, x, in_u8=in_u8, aligned=aligned, out_shift=shift)
            h.close()
            _same(got, want, "n_in %d, %s rows, output %d floats past a boundary" % (n, "aligned" if aligned else "odd", shift))


@pytest.mark.parametrize("mode", [FM, PM, AM], ids=["fm", "pm", "am"])
def test_the_exact_values_and_the_denormal_pair(api, mode):
    """The table alone, at every place in a group of four and across the head peel."""
    for lead in range(5):
        x = np.concatenate([np.full(lead, 0.5 - 0.25j, np.complex64), TABLE, TABLE[::-1]])[None, :]
        want = _plan(api, x, mode, False, gain=1.0)
        h = api.Polar(mode, 1.0)
        _same(run_polar(api, h, x, out_shift=lead % 4), want, "table behind %d samples" % lead)
        h.close()
    if mode == PM:
        pi_2, pi = np.float32(float.fromhex("0x1.921fb6p+0")), np.float32(float.fromhex("0x1.921fb6p+1"))
        assert np.array_equal(_bits(want[0, 4:9]), _bits([0.0, 0.0, pi_2, -pi_2, pi]))       # lead 4: the table's first entries
        assert abs(float(want[0, 4 + 10]) - np.arctan(0.1)) < 1e-5                            # the denormal pair: z = 0.1


# ------------------------------------------------------------------------------------------------ the contracts about bits
@pytest.mark.parametrize("in_u8", [False, True], ids=["cf32", "u8"])
def test_cutting_the_stream_gives_the_same_bits(api, L, in_u8):
    n = 1 + 3 + 1020 + 5 + 2071
    x = _bytes(n, 2, seed=3) if in_u8 else _streams(n, 2)
    want = _plan(api, x, FM, in_u8)
    for aligned in (True, False):
        one = api.Polar(FM, GAIN, n_streams=2)
        cut = api.Polar(FM, GAIN, n_streams=2)
        if in_u8:
            one.set_input_format(L.FMT_U8)
            cut.set_input_format(L.FMT_U8)
        a = run_polar(api, one, x, in_u8=in_u8, aligned=aligned)
        b = run_polar(api, cut, x, cuts=[1, 3, 1020, 5, 2071], in_u8=in_u8, aligned=aligned, out_shift=1)
        _same(a, want, "one call")
        _same(b, a, "calls of 1, 3, 1020, 5 and the rest")
    # sample by sample: every call is a head peel that reads the carried sample and leaves the next one
    h = api.Polar(FM, GAIN, n_streams=2)
    if in_u8:
        h.set_input_format(L.FMT_U8)
    m = 40
    _same(run_polar(api, h, x[:, :(2 if in_u8 else 1) * m], cuts=[1] * m, in_u8=in_u8), want[:, :m], "calls of one sample")


def test_the_format_may_change_between_calls(api, L):
    n, cut = 3001, 1234
    b = _bytes(n, 2, seed=9)
    xf = np.stack([synth.u8_to_cf32(r) for r in b])
    want = _plan(api, b, FM, True)
    _same(_plan(api, xf, FM, False), want, "the plans of the two formats")
    h = api.Polar(FM, GAIN, n_streams=2)
    h.set_input_format(L.FMT_U8)
    first = run_polar(api, h, b[:, :2 * cut], in_u8=True, aligned=False)
    h.set_input_format(L.FMT_F32)
    second = run_polar(api, h, xf[:, cut:], aligned=False, out_shift=3)
    _same(np.concatenate([first, second], axis=1), want, "u8 then cf32")
    h.set_input_format(L.FMT_U8)                                  # and back: the stream goes on where it was
    third = run_polar(api, h, b[:, :2 * cut], in_u8=True)
    _same(third[:, 1:], want[:, 1:cut], "u8 again")
    assert not np.array_equal(_bits(third[:, 0]), _bits(want[:, 0]))     # its first sample followed the last one of `second`


def test_streams_are_independent_and_reset_makes_a_fresh_handle(api):
    n = 4099
    x = _streams(n, 3)
    h = api.Polar(FM, GAIN, n_streams=3)
    fresh = run_polar(api, h, x, aligned=False)
    _same(fresh, _plan(api, x, FM, False), "three streams")
    alone = api.Polar(FM, GAIN)
    _same(run_polar(api, alone, x[1:2]), fresh[1:2], "stream 1 of 3 against a handle of its own")
    # without a reset the stream goes on: the first output follows the last sample of the call before
    again = run_polar(api, h, x, aligned=False)
    assert not np.array_equal(_bits(again[:, 0]), _bits(fresh[:, 0]))
    _same(again[:, 1:], fresh[:, 1:], "the second pass, from its second sample on")
    h.reset()
    _same(run_polar(api, h, x, aligned=False), fresh, "after reset")
    for s in range(3):
        want0 = api.polar_plan(x[s, :1], FM, GAIN, prev=x[s, -1])[0]
        _same(again[s, :1], want0, "the carried sample of stream %d" % s)


def test_the_same_calls_give_the_same_bits_every_run(api):
    x = _streams(65539, 2)
    runs = []
    for _ in range(2):
        h = api.Polar(FM, GAIN, n_streams=2)
        runs.append(run_polar(api, h, x, cuts=[4099, 61440], aligned=False))
        h.close()
    _same(runs[1], runs[0], "second run")


# ------------------------------------------------------------------------------------------------ capture
class Hip:
    """The HIP graph calls a capturing caller makes, through libamdhip64 (the product library is not involved)."""

    def __init__(self):
        self.h = C.CDLL("libamdhip64.so")
        vp, pvp, psz = C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)
        for name, args in (("hipStreamCreate", [pvp]), ("hipStreamBeginCapture", [vp, C.c_int]), ("hipStreamEndCapture", [vp, pvp]),
                           ("hipGraphInstantiate", [pvp, vp, vp, vp, C.c_size_t]), ("hipGraphLaunch", [vp, vp]),
                           ("hipStreamSynchronize", [vp]), ("hipGraphExecDestroy", [vp]), ("hipGraphDestroy", [vp]),
                           ("hipStreamDestroy", [vp]), ("hipGraphGetNodes", [vp, pvp, psz]), ("hipGraphGetRootNodes", [vp, pvp, psz]),
                           ("hipGraphGetEdges", [vp, pvp, pvp, psz])):
            fn = getattr(self.h, name)
            fn.argtypes, fn.restype = args, C.c_int

    def ok(self, rc):
        assert rc == 0, "HIP error %d" % rc

    def capture(self, body):
        s = C.c_void_p()
        self.ok(self.h.hipStreamCreate(C.byref(s)))
        self.ok(self.h.hipStreamBeginCapture(s, 0))          # hipStreamCaptureModeGlobal
        try:
            body(s.value)
        finally:
            g = C.c_void_p()
            rc = self.h.hipStreamEndCapture(s, C.byref(g))
        self.ok(rc)
        ex = C.c_void_p()
        self.ok(self.h.hipGraphInstantiate(C.byref(ex), g, None, None, 0))
        return s, g, ex

    def shape(self, g):
        """(nodes, roots, the edges as (from, to) pairs) of a graph."""
        n, r, e = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        self.ok(self.h.hipGraphGetNodes(g, None, C.byref(n)))
        self.ok(self.h.hipGraphGetRootNodes(g, None, C.byref(r)))
        self.ok(self.h.hipGraphGetEdges(g, None, None, C.byref(e)))
        frm, to = (C.c_void_p * max(1, e.value))(), (C.c_void_p * max(1, e.value))()
        if e.value:
            self.ok(self.h.hipGraphGetEdges(g, frm, to, C.byref(e)))
        return n.value, r.value, [(frm[i], to[i]) for i in range(e.value)]

    def free(self, s, g, ex):
        self.h.hipGraphExecDestroy(ex)
        self.h.hipGraphDestroy(g)
        self.h.hipStreamDestroy(s)


def test_a_captured_call_replays_the_next_chunks(api, L):
    env = dict(os.environ)
    hip = Hip()
    S, n, si, so = 2, 4099, 4101, 4103
    x = _streams(6 * n, S, table=False)
    want = _plan(api, x, FM, False)
    chunk = lambda i: x[:, i * n:(i + 1) * n]
    h = api.Polar(FM, GAIN, n_streams=S)
    d_in = sc.device_array(api, 2 * S * si)
    d_out = sc.device_array(api, S * so + 1)
    out = d_out.ptr + 4                                       # one float past a boundary: a head peel in every replay

    def put(i, stream=None):
        pad = np.zeros((S, si), np.complex64)
        pad[:, :n] = chunk(i)
        api.check(L.load().sfe_dsp_memcpy_h2d(d_in.ptr, pad.ctypes.data, pad.nbytes, stream))
        api.check(L.load().sfe_dsp_sync(stream))

    def take(i, what, stream=None):
        y = d_out.to_numpy(S * so, offset=1, stream=stream).reshape(S, so)
        _same(y[:, :n], want[:, i * n:(i + 1) * n], what)
        assert (y[:, n:].view(np.uint32) == sc.POISON).all(), what      # the gap between the rows

    put(0)
    assert h.process_stream(d_in.ptr, n, out, in_stride=si, out_stride=so) == n            # eager: chunk 0
    api.sync()
    take(0, "the eager call before the capture")
    ks = []
    s, g, ex = hip.capture(lambda st: ks.append(h.process_stream(d_in.ptr, n, out, in_stride=si, out_stride=so, stream=st)))
    assert ks == [n]
    nodes, roots, edges = hip.shape(g)
    print("polar captured call: %d nodes, %d root(s), %d edges" % (nodes, roots, len(edges)))
    assert nodes >= 1 and roots == 1 and len(edges) == nodes - 1                            # the graph is linear:
    assert len({a for a, _ in edges}) == len(edges) and len({b for _, b in edges}) == len(edges)   # no node has two successors
    # the capture ran nothing: chunk 1 is still to come.  Replay, replay, an eager call in between, replay
    for i, kind in ((1, "g"), (2, "g"), (3, "e"), (4, "g")):
        if kind == "g":
            put(i, s.value)
            hip.ok(hip.h.hipGraphLaunch(ex, s))
            hip.ok(hip.h.hipStreamSynchronize(s))
            take(i, "replay of chunk %d" % i, s.value)
        else:
            put(i)
            assert h.process_stream(d_in.ptr, n, out, in_stride=si, out_stride=so) == n
            api.sync()
            take(i, "the eager call between the replays")
    hip.free(s, g, ex)
    put(5)
    assert h.process_stream(d_in.ptr, n, out, in_stride=si, out_stride=so) == n            # and the stream goes on without the graph
    api.sync()
    take(5, "the eager call behind the replays")
    h.close()
    assert dict(os.environ) == env                            # the runtime's queue settings, and everything else, as they were


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_launch_nothing(api, L):
    lib = L.load()
    n, S = 1024, 2
    x = _streams(n, S)
    d_in = sc.from_numpy(api, np.concatenate([x.view(np.float32).ravel(), np.zeros(64, np.float32)]))
    d_out = sc.device_array(api, S * n + 64)
    h = api.Polar(FM, GAIN, n_streams=S)
    k = C.c_size_t(7)

    def call(pi, n_in, in_stride, po, out_stride, handle=None):
        k.value = 7
        rc = lib.sfe_dsp_polar_process_stream(handle or h._h, pi, n_in, in_stride, po, out_stride, C.byref(k), None)
        if rc != L.SFE_OK:
            assert k.value == 0 and lib.sfe_dsp_last_error().startswith(b"polar_process_stream: "), lib.sfe_dsp_last_error()
        return rc

    assert call(d_in.ptr + 4, n, n, d_out.ptr, n) == L.SFE_EINVAL                 # cf32 wants 8 bytes
    assert call(d_in.ptr, n, n, d_out.ptr + 2, n) == L.SFE_EINVAL                 # float32 wants 4
    assert call(d_in.ptr, n, n, d_out.ptr, n - 1) == L.SFE_ERANGE                 # out_stride one sample short
    assert call(d_in.ptr, n, n - 1, d_out.ptr, n) == L.SFE_EINVAL                 # in_stride short with two streams
    assert call(None, n, n, d_out.ptr, n) == L.SFE_EINVAL
    assert call(d_in.ptr, n, n, None, n) == L.SFE_EINVAL
    assert call(d_in.ptr, n, n, d_in.ptr + 8 * n, n) == L.SFE_EINVAL              # the output inside the input's range
    assert call(d_in.ptr, n, n, d_in.ptr + 8 * S * n - 4, n) == L.SFE_EINVAL      # ... and over its last word
    assert call(d_in.ptr, 1 << 31, 1 << 31, d_out.ptr, 1 << 31) == L.SFE_EINVAL   # n_in >= 2^31
    assert call(d_in.ptr, n, 1 << 62, d_out.ptr, n) == L.SFE_EINVAL               # a stride that leaves the address space
    h.set_input_format(L.FMT_U8)
    assert call(d_in.ptr + 1, n, n, d_out.ptr, n) == L.SFE_EINVAL                 # byte pairs want 2
    assert lib.sfe_dsp_polar_set_input_format(h._h, 7) == L.SFE_EINVAL            # a bad format: the handle stays u8
    assert lib.sfe_dsp_polar_set_input_format(h._h, L.FMT_TX10) == L.SFE_EINVAL
    assert lib.sfe_dsp_last_error().startswith(b"polar: ")
    assert h.in_u8
    h.set_input_format(L.FMT_F32)
    assert call(d_in.ptr, 0, n, d_out.ptr, n) == L.SFE_OK and k.value == 0        # n_in = 0: a no-op, even with null buffers
    assert call(None, 0, 0, None, 0) == L.SFE_OK and k.value == 0
    api.sync()
    assert (d_out.to_numpy(keep=True).view(np.uint32) == sc.POISON).all()         # nothing was stored; check_guarded holds the rest
    # nothing advanced either: the next good call is a fresh handle's
    assert call(d_in.ptr, n, n, d_out.ptr, n) == L.SFE_OK and k.value == n
    api.sync()
    _same(d_out.to_numpy(S * n).reshape(S, n), _plan(api, x, FM, False), "after the refusals")
    h.close()


# ------------------------------------------------------------------------------------------------ behind the down-converter
def test_ddc_rows_are_read_in_place(api):
    """Ddc with K = 2 writes its rows on the device, Polar FM with n_streams = 2 reads those rows where they lie."""
    decim, n_out = 8, 1500
    stride = 1507
    x = synth.synth_cf32(decim * n_out, ch=3).view(np.complex64)
    ddc = api.Ddc(synth.lowpass_taps(64, 0.05), decim, [0.1, -0.2])
    d_x = sc.from_numpy(api, x.view(np.float32))
    d_mid = sc.device_array(api, 2 * 2 * stride)
    d_y = sc.device_array(api, 2 * stride + 3)
    assert ddc.process_stream(d_x.ptr, decim * n_out, d_mid.ptr, out_stride=stride) == n_out
    fm = api.Polar(FM, 0.25, n_streams=2)
    assert fm.process_stream(d_mid.ptr, n_out, d_y.ptr + 12, in_stride=stride, out_stride=stride) == n_out
    api.sync()
    mid = d_mid.to_numpy(keep=True).view(np.complex64).reshape(2, stride)
    y = d_y.to_numpy(2 * stride, offset=3).reshape(2, stride)
    assert (mid[:, n_out:].view(np.uint32) == sc.POISON).all() and (y[:, n_out:].view(np.uint32) == sc.POISON).all()
    rows = np.ascontiguousarray(mid[:, :n_out])
    assert np.isfinite(rows.view(np.float32)).all() and np.abs(rows).max() > 1e-3
    _same(y[:, :n_out], _plan(api, rows, FM, False, gain=0.25), "FM of the two tunings")
    # the detector changed nothing it read: a second download of the rows is the first
    assert np.array_equal(d_mid.to_numpy(keep=True).view(np.uint32), mid.view(np.uint32).ravel())
    fm.close()
    ddc.close()
