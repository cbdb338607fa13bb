"""What the six streaming blocks (chan, combine, ddc, psd, corr, iir) share on the host side (csrc/block.h), at the
smallest shapes each accepts: the refusal of a capturing stream, the refusal of another block's handle, the caller's
current device across create, and the grow-only scratch of psd, corr and iir.  Everything is compared bit for bit with
what a fresh handle gives; the arithmetic itself is the business of the blocks' own tests.  `-m gpu`."""
import ctypes as C

import numpy as np
import pytest

from simplefe_amd import synth

pytestmark = pytest.mark.gpu
SENT = 7.0


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
                       ("hipStreamDestroy", [C.c_void_p]), ("hipGetDevice", [C.POINTER(C.c_int)]), ("hipSetDevice", [C.c_int])):
        fn = getattr(h, name)
        fn.argtypes, fn.restype = args, C.c_int
    return h


def _cf32(n, ch=0):
    return synth.synth_cf32(n, ch=ch)           # 2n floats, (re, im) interleaved


class Block:
    """One block at its smallest shape: how to make a handle, one good call's input (float32 values as uploaded), the
    float32 slots of its outputs (dense: the call writes every one), and the arguments of sfe_dsp_<prefix>_process_stream
    between the handle and the counter."""

    def __init__(self, prefix, new, x, outs, args, counted, setter="set_input_format"):
        self.prefix, self.new, self.x, self.outs, self.args, self.counted, self.setter = prefix, new, x, outs, args, counted, setter

    def fn(self, L, name):
        return getattr(L.load(), "sfe_dsp_%s_%s" % (self.prefix, name))

    def buffers(self, api):
        return api.DeviceArray.from_numpy(self.x), [api.DeviceArray.from_numpy(np.full(n, SENT, np.float32)) for n in self.outs]

    def call(self, L, handle, d_in, d_outs, k, stream=None):
        return self.fn(L, "process_stream")(handle, *self.args(d_in.ptr, [d.ptr for d in d_outs]), C.byref(k), stream)


def _chan(half):
    M, D, n = 4, 2 if half else 4, 64
    h = synth.lowpass_taps(4 * M, 1.0 / M)
    return Block("chan", lambda api, device=0: api.Chan(h, M, D, device=device), _cf32(n * D), [2 * M * n],
                 lambda pi, po: (pi, n * D, n * D, po[0], n), n)


def _combine(half):
    M, D, n = 4, 2 if half else 4, 64
    g = synth.lowpass_taps(4 * M, 1.0 / M)
    return Block("combine", lambda api, device=0: api.Combiner(g, M, D, device=device), _cf32(M * n), [2 * n * D],
                 lambda pi, po: (pi, n, n, po[0], n * D), n * D, setter="set_output_format")


def _ddc():
    D, K, n = 3, 2, 64
    h = synth.lowpass_taps(8 * D, 0.5 / D)
    return Block("ddc", lambda api, device=0: api.Ddc(h, D, [0.125, -0.3], device=device), _cf32(n * D), [2 * K * n],
                 lambda pi, po: (pi, n * D, n * D, po[0], n), n)


def _psd(n_avg=2, segs=8):
    N, hop = 256, 128
    w = np.hanning(N).astype(np.float32)
    rows = segs // n_avg
    return Block("psd", lambda api, device=0: api.Psd(w, hop, n_avg, device=device), _cf32(segs * hop), [rows * N],
                 lambda pi, po: (pi, segs * hop, segs * hop, po[0], rows * N), rows)


CORR_LEN = 257
CORR_V = 4096 - 256 * -(-(CORR_LEN - 1) // 256)        # the transform advance of this length
CORR_B = 2 * CORR_V                                    # block > advance: the call keeps slot peaks in scratch


def _corr_templates(K=2):
    t = np.stack([_cf32(CORR_LEN, ch=100 + k).view(np.complex64) for k in range(K)])
    return (np.where(t.real >= 0, 1.0, -1.0) + 1j * np.where(t.imag >= 0, 1.0, -1.0)).astype(np.complex64)


def _corr(blocks=2):
    """The shape of test_gpu_corr.py::test_refusals_launch_nothing."""
    K, n = 2, blocks * CORR_B
    t = _corr_templates(K)
    return Block("corr", lambda api, device=0: api.Corr(t, CORR_B, 1e-6, device=device), _cf32(n), [K * blocks, K * blocks, K * n],
                 lambda pi, po: (pi, n, n, po[0], po[1], blocks, po[2], n), blocks)


def _iir(blocks=1):
    from simplefe_amd import api
    sos = synth.iir_dc_blocker(0.995)
    n = blocks * api.iir_plan(sos)[0]
    return Block("iir", lambda api, device=0: api.Iir(sos, device=device), _cf32(n), [2 * n], lambda pi, po: (pi, n, n, po[0], n), n)


BLOCKS = {"chan": lambda: _chan(False), "chan-half": lambda: _chan(True), "combine": lambda: _combine(False),
          "combine-half": lambda: _combine(True), "ddc": _ddc, "psd": _psd, "corr": _corr, "iir": _iir}


def _bits(d_outs):
    return [d.to_numpy().view(np.uint32) for d in d_outs]


def _fresh_bits(api, L, b):
    """The outputs of one good call on a new handle."""
    obj = b.new(api)
    d_in, d_outs = b.buffers(api)
    k = C.c_size_t(0)
    assert b.call(L, obj._h, d_in, d_outs, k) == L.SFE_OK and k.value == b.counted
    return _bits(d_outs)


def _same(got, want):
    return len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want))


def _untouched(d_outs):
    return all(np.all(d.to_numpy() == SENT) for d in d_outs)


@pytest.mark.parametrize("name", list(BLOCKS))
def test_capturing_stream_is_refused(api, L, hip, name):
    """The counters and the carried pair advance on the host: a call on a capturing stream is SFE_ESTATE, counts nothing,
    enqueues nothing and moves nothing, so the next ordinary call gives what a fresh handle gives."""
    b = BLOCKS[name]()
    obj = b.new(api)
    d_in, d_outs = b.buffers(api)
    k = C.c_size_t(5)
    s = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(s)) == 0
    assert hip.hipStreamBeginCapture(s, 2) == 0            # relaxed mode: the refused call launches nothing
    try:
        rc = b.call(L, obj._h, d_in, d_outs, k, s.value)
    finally:
        g = C.c_void_p()
        hip.hipStreamEndCapture(s, C.byref(g))
    if g.value:
        hip.hipGraphDestroy(g)
    hip.hipStreamDestroy(s)
    assert rc == L.SFE_ESTATE and k.value == 0
    assert b"graph capture is not supported" in L.load().sfe_dsp_last_error()
    api.sync()
    assert _untouched(d_outs)
    assert b.call(L, obj._h, d_in, d_outs, k) == L.SFE_OK and k.value == b.counted
    assert _same(_bits(d_outs), _fresh_bits(api, L, b))


# a live handle of block A handed to the functions of block B; every block is A once and B once
FOREIGN = [("chan", "combine"), ("combine", "ddc"), ("ddc", "psd"), ("psd", "corr"), ("corr", "iir"), ("iir", "chan")]


@pytest.mark.parametrize("name_a,name_b", FOREIGN)
def test_foreign_handle_is_refused(api, L, name_a, name_b):
    """Each handle starts with its block's own magic word: B's functions refuse A's live handle with SFE_EINVAL, touch no
    buffer and nothing of A, and B's destroy on it is SFE_OK and frees nothing -- A then gives a fresh handle's bits."""
    a, b = BLOCKS[name_a](), BLOCKS[name_b]()
    obj = a.new(api)
    d_in, d_outs = b.buffers(api)
    k = C.c_size_t(5)
    assert b.fn(L, b.setter)(obj._h, L.FMT_F32) == L.SFE_EINVAL
    assert b.call(L, obj._h, d_in, d_outs, k) == L.SFE_EINVAL and k.value == 0
    assert b.fn(L, "reset")(obj._h) == L.SFE_EINVAL
    assert b.fn(L, "destroy")(obj._h) == L.SFE_OK
    api.sync()
    assert _untouched(d_outs) and np.array_equal(d_in.to_numpy(b.x.size), b.x)
    a_in, a_outs = a.buffers(api)
    assert a.call(L, obj._h, a_in, a_outs, k) == L.SFE_OK and k.value == a.counted
    assert _same(_bits(a_outs), _fresh_bits(api, L, a))


def test_create_leaves_the_current_device(api, L, hip):
    """create runs on the handle's device and puts the caller's current device back, whether it succeeds or refuses."""
    def current():
        d = C.c_int(-1)
        assert hip.hipGetDevice(C.byref(d)) == 0
        return d.value

    n_dev = api.device_count()
    assert hip.hipSetDevice(0) == 0
    for name in ("chan", "combine", "ddc", "psd", "corr", "iir"):
        b = BLOCKS[name]()
        for device in range(min(n_dev, 2)):
            obj = b.new(api, device)
            assert current() == 0, (name, device)
            obj.close()
            assert current() == 0, (name, device)
        with pytest.raises(api.SfeError):
            b.new(api, n_dev)                   # out of range: refused before anything is allocated
        assert current() == 0, name


# a call of g granules on one handle shape.  psd: n_avg = 3 (up to n_avg = 2 a chunk of the summation order is a whole
# row and a call needs no scratch), a granule is one row; corr: a block of two advances; iir: its block
GROW = {"psd": lambda g: _psd(3, 3 * g), "corr": _corr, "iir": _iir}


def _run_cuts(api, L, make, obj, d_in, cuts):
    """Consecutive pieces of d_in, cuts[i] granules each, through handle obj; the bits of every call's outputs."""
    got, pos = [], 0
    for g in cuts:
        b = make(g)
        d_outs = [api.DeviceArray.from_numpy(np.full(m, SENT, np.float32)) for m in b.outs]
        k = C.c_size_t(0)
        rc = b.fn(L, "process_stream")(obj._h, *b.args(d_in.ptr + 4 * pos, [d.ptr for d in d_outs]), C.byref(k), None)
        assert rc == L.SFE_OK and k.value == b.counted
        got.append(_bits(d_outs))
        pos += b.x.size
    return got


@pytest.mark.parametrize("name", list(GROW))
def test_scratch_grows_and_is_kept(api, L, name):
    """The scratch of one call is allocated when a longer call than any before arrives and kept from then on.  A small, a
    longer and a small call on a new handle give the bits of the same three calls on a handle whose scratch a longer call
    had sized before (and which was reset): neither growing in mid-stream nor the larger table changes a value."""
    make = GROW[name]
    cuts = [1, 4, 1]
    d_in = api.DeviceArray.from_numpy(make(sum(cuts)).x)
    grown = _run_cuts(api, L, make, make(1).new(api), d_in, cuts)
    first = make(1).new(api)
    _run_cuts(api, L, make, first, d_in, [4])
    first.reset()
    kept = _run_cuts(api, L, make, first, d_in, cuts)
    assert all(_same(g, w) for g, w in zip(grown, kept))
    assert _same(grown[0], _fresh_bits(api, L, make(1)))        # and the first call is a fresh handle's
