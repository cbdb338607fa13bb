"""The burst modulator (sfe_dsp_mod_*) on the GPU.  The bar is equality with api.mod_plan -- float32 words or wire-format
bytes -- never a tolerance.  Every output sits between guards and is poisoned before every call (the poison and guard idea
of tests/stream_checks.py): after the call no poison is left in the stream's n_out samples and the guards are intact.  The
grid of tests/test_mod_host.py, frames far longer than a tile, the contracts about bits checked literally, a captured call,
the refusals, a relay behind a real decoder, and the loopback Mod -> Corr -> Burst -> Vit, all on the device."""
import ctypes as C

import numpy as np
import pytest

import mod_checks as mc
import stream_checks as sc
from simplefe_amd import synth

pytestmark = pytest.mark.gpu
F32 = np.float32
GUARD = 64                          # bytes before and behind the output
K7 = (7, (0o171, 0o133))


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
        same = raw == np.full(self.words, sc.POISON, np.uint32).view(np.uint8)
        assert same[:self.front].all() and same[self.front + self.nbytes:].all(), "a store outside the stream"
        cell = 5 if self.tx10 else 4
        body = same[self.front:self.front + self.nbytes]
        # a cell that kept all its poison bytes was never stored (no sample's word, and no group of the wire format, looks like it)
        kept = np.array([body[i::cell][:self.nbytes // cell] for i in range(cell)]).all(axis=0)
        assert not kept.any(), "%d cells of the stream were never stored, the first at %d" % (int(kept.sum()), int(np.flatnonzero(kept)[0]))
        got = raw[self.front:self.front + self.nbytes].copy()
        return got if self.tx10 else got.view(np.complex64)

    def free(self):
        self.d.free()


def run(api, h, data, n_out, start_base=0, start_step=0, in_pad=0, lead=0, shift=0, call=None):
    """One call: burst b's bytes `lead` bytes into their buffer and in_pad bytes apart; returns the stream."""
    data = np.ascontiguousarray(np.atleast_2d(data), np.uint8)
    nb, stride = data.shape[0], data.shape[1] + in_pad
    buf = np.full(lead + nb * stride + 3, 0x5A, np.uint8)
    for b in range(nb):
        buf[lead + b * stride:][:data.shape[1]] = data[b]
    d_in = api.DeviceArray.from_bytes(buf)
    out = Out(api, n_out, h.out_fmt == 2, shift)
    try:
        k = (call or h.process_stream)(d_in.ptr + lead, nb, out.ptr, n_out, start_base, start_step, in_stride=stride)
        api.sync()
        assert k == n_out
        return out.take()
    finally:
        d_in.free()
        out.free()


def same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got.view(np.uint8), want.view(np.uint8))


def dyadic_taps(n, seed):
    return (np.random.default_rng(seed).integers(-1024, 1025, size=n) / 1024.0).astype(F32)


def both_formats(L):
    return ((L.FMT_F32, 8), (L.FMT_TX10, 3))          # (format, the output's byte offset from a 64-byte boundary)


# ---- the grid of the host tests
@pytest.mark.parametrize("code", mc.CODES + [(7, None)], ids=mc.CODE_IDS + ["uncoded"])
@pytest.mark.parametrize("terminated", [True, False], ids=["terminated", "truncated"])
def test_codes_equal_the_plan(api, L, code, terminated):
    """Every code, punctured and not, BPSK and QPSK (an odd n_soft among them), at n_info 1, 5, 64 and 200: one burst and
    seven, F32 and TX10, behind a one-symbol preamble and a five-tap pulse at two samples per symbol."""
    K, gen = code
    taps, pre = dyadic_taps(5, 1), np.array([0.5 - 0.25j], np.complex64)
    for n_info in (1, 5, 64, 200):
        data = mc.payload_bytes(n_info, 7, n_info + K)
        for keep in (None, mc.PUNCT[len(gen)]) if gen else (None,):
            for order in (2, 4):
                for fmt, shift in both_formats(L):
                    kw = dict(keep=keep, terminated=terminated, order=order, preamble=pre, amp=0.5, out_fmt=fmt)
                    h = api.Mod(K, gen, n_info, taps, 2, **kw)
                    F = h.frame_len
                    for nb in (1, 7):
                        place = dict(n_out=nb * (F + 3) + 12 + nb * (F + 3) % 2, start_base=5, start_step=F + 3)
                        want = api.mod_plan(K, gen, n_info, taps, 2, data=data[:nb], **kw, **place)
                        assert same(run(api, h, data[:nb], in_pad=n_info % 3, lead=1, shift=shift, **place), want), (n_info, keep, order, fmt, nb)
                    h.close()


SHAPES = [(1, 1, 0), (2, 3, 1), (10, 3, 32), (4, 7, 1), (10, 161, 32), (64, 3, 0), (1, 64, 1), (2, 128, 32), (64, 4096, 1), (7, 40, 3)]


@pytest.mark.parametrize("shape", SHAPES, ids=["sps%d-taps%d-pre%d" % s for s in SHAPES])
def test_shapes_and_placements_equal_the_plan(api, L, shape):
    """Every pulse and preamble length of the host grid; frames that touch (start_step = F) and frames F + 3 apart, an odd
    start_base, a tail behind the last frame; one burst and seven; F32 at both 16-byte phases of its address, TX10."""
    sps, n_taps, Lp = shape
    K, gen = K7
    n_info, keep = 45, mc.PUNCT[2]
    rng = np.random.default_rng(n_taps)
    taps, pre = dyadic_taps(n_taps, n_taps), ((rng.integers(-64, 65, Lp) + 1j * rng.integers(-64, 65, Lp)) / 64.0).astype(np.complex64)
    data = mc.payload_bytes(n_info, 7, sps)
    for fmt, shift in both_formats(L) + ((L.FMT_F32, 0),):
        kw = dict(keep=keep, preamble=pre, amp=0.5, out_fmt=fmt)
        h = api.Mod(K, gen, n_info, taps, sps, **kw)
        F = h.frame_len
        for nb, base, step, tail in ((1, 0, 0, 0), (1, 3, 0, 5), (7, 0, F, 0), (7, 9, F, 2), (7, 13, F + 3, 21), (7, 2, F + 2000, 2)):
            n_out = base + (nb - 1) * step + F + tail
            place = dict(n_out=n_out + n_out % 2, start_base=base, start_step=step)
            want = api.mod_plan(K, gen, n_info, taps, sps, data=data[:nb], **kw, **place)
            assert same(run(api, h, data[:nb], in_pad=2, lead=3, shift=shift, **place), want), (fmt, nb, base, step)
        h.close()


def test_no_bursts_write_zeros(api, L):
    for fmt, shift in both_formats(L):
        h = api.Mod(7, None, 8, [1.0], 1, out_fmt=fmt)
        got = run(api, h, np.zeros((0, 1), np.uint8), 3000, shift=shift)
        assert same(got, api.mod_plan(7, None, 8, [1.0], 1, out_fmt=fmt, data=np.zeros((0, 1), np.uint8), n_out=3000))
        assert not got.view(np.uint8).any() if fmt == L.FMT_F32 else (got.reshape(-1, 5) == [0xAA, 0, 0, 0, 0]).all()
        h.close()


# ---- frames far longer than a tile
LONG = [dict(K=9, gen=(0o765, 0o671, 0o513, 0o473), n_info=8192, order=4, sps=2, n_taps=33, Lp=32),
        dict(K=7, gen=K7[1], n_info=200, order=2, sps=64, n_taps=4096, Lp=0),
        dict(K=7, gen=K7[1], n_info=2000, order=2, sps=1, n_taps=64, Lp=1),
        dict(K=7, gen=K7[1], n_info=500, order=4, sps=10, n_taps=161, Lp=32)]


@pytest.mark.parametrize("s", LONG, ids=["K9n4-8192-qpsk-sps2", "sps64-Q64", "sps1-Q64", "sps10-Q17"])
def test_long_frames_equal_the_plan(api, L, s):
    """Frames of at least three tiles, cut wherever the tiles fall: at sps 64 and Q = 64 a tile holds 16 symbols, so every
    tile edge cuts the 63-symbol halo and each q reaches across one; two bursts, an odd start_base, F32 and TX10."""
    tile, _ = api.mod_footprint()
    taps = mc.rc_taps(10, 8) if s["n_taps"] == 161 else dyadic_taps(s["n_taps"], 4)
    pre = synth.psk_symbols(s["Lp"], 4, seed=2).astype(np.complex64)
    data = mc.payload_bytes(s["n_info"], 2, 77)
    for fmt, shift in both_formats(L):
        kw = dict(order=s["order"], preamble=pre, amp=0.5, out_fmt=fmt)
        h = api.Mod(s["K"], s["gen"], s["n_info"], taps, s["sps"], **kw)
        F = h.frame_len
        assert F >= 3 * tile and (s["sps"] != 64 or tile // s["sps"] < 63)
        place = dict(n_out=2 * F + 1 + 777 + 12, start_base=777, start_step=F + 1)
        want = api.mod_plan(s["K"], s["gen"], s["n_info"], taps, s["sps"], data=data, **kw, **place)
        assert same(run(api, h, data, shift=shift, **place), want), fmt
        h.close()


# ---- the contracts about bits
@pytest.mark.parametrize("fmt", ["f32", "tx10"])
def test_runs_repeat_and_a_frame_depends_on_its_bytes_alone(api, L, fmt):
    """The same call twice; every burst of a 70-burst call against a one-burst call at another address, stride and offset."""
    K, gen = K7
    n_info, keep, sps = 61, mc.PUNCT[2], 4
    taps, pre = mc.rc_taps(4, 3), synth.psk_symbols(5, 4, seed=1).astype(np.complex64)
    kw = dict(keep=keep, preamble=pre, amp=0.5, out_fmt=L.FMT_TX10 if fmt == "tx10" else L.FMT_F32)
    h = api.Mod(K, gen, n_info, taps, sps, **kw)
    F = h.frame_len
    data = mc.payload_bytes(n_info, 70, 5)
    step = F + 6                                                 # even: every frame has the same phase in its 5-byte groups
    place = dict(n_out=70 * step + 10, start_base=4, start_step=step)
    a = run(api, h, data, in_pad=3, lead=2, shift=8, **place)
    b = run(api, h, data, in_pad=3, lead=2, shift=8, **place)
    assert same(a, b) and same(a, api.mod_plan(K, gen, n_info, taps, sps, data=data, **kw, **place))
    per = 5 if fmt == "tx10" else 2                              # bytes, or complex samples, per two samples
    for i in range(70):
        base = 2 * (i % 5) + 6
        one = run(api, h, data[i], in_pad=i % 4, lead=1 + i % 3, shift=(i % 2) * 8 if fmt == "f32" else i % 7, n_out=base + F + 6,
                  start_base=base)
        assert np.array_equal(one[base // 2 * per:][:F // 2 * per], a[(4 + i * step) // 2 * per:][:F // 2 * per]), i
    h.close()


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
    K, gen = K7
    n_info, taps, sps = 106, mc.rc_taps(10, 8), 10
    data = mc.payload_bytes(n_info, 3, 9)
    h = api.Mod(K, gen, n_info, taps, sps, amp=0.5)
    F = h.frame_len
    place = dict(n_out=3 * F + 40, start_base=11, start_step=F + 7)
    want = api.mod_plan(K, gen, n_info, taps, sps, amp=0.5, data=data, **place)
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
    K, gen = K7
    n_info, nb, sps = 64, 3, 4
    taps = mc.rc_taps(4, 2)
    h = api.Mod(K, gen, n_info, taps, sps, amp=0.5)
    ht = api.Mod(K, gen, n_info, taps, sps, amp=0.5, out_fmt=L.FMT_TX10)
    F, nbytes = h.frame_len, h.n_bytes
    assert (h.n_sym, F, nbytes) == (140, (140 + 5 - 1) * 4, 8)
    data = mc.payload_bytes(n_info, nb, 41)
    n_out = nb * F + 6
    d_in = api.DeviceArray.from_bytes(np.concatenate([data.ravel(), np.zeros(64, np.uint8)]))
    out = Out(api, n_out, False, 0)
    lib = L.load()
    k = C.c_size_t(7)

    def call(pi=d_in.ptr, istride=nbytes, n_bursts=nb, base=2, step=F, po=out.ptr, n=n_out, hh=h._h, kk=C.byref(k)):
        return lib.sfe_dsp_mod_process_stream(hh, pi, istride, n_bursts, base, step, po, n, kk, None)

    assert call(istride=nbytes - 1) == L.SFE_ERANGE and lib.sfe_dsp_last_error().startswith(b"mod_process_stream: ")
    assert call(pi=None) == L.SFE_EINVAL and call(po=None) == L.SFE_EINVAL
    assert call(po=out.ptr + 4) == L.SFE_EINVAL                      # cf32 output is eight-byte aligned
    assert call(base=-1) == L.SFE_EINVAL and call(step=F - 1) == L.SFE_EINVAL
    assert call(base=7) == L.SFE_EINVAL and call(n=n_out - 5) == L.SFE_EINVAL     # the last frame would end behind the stream
    assert call(n=1 << 31) == L.SFE_EINVAL and call(n_bursts=1 << 31) == L.SFE_EINVAL
    assert call(hh=ht._h, n=n_out - 1) == L.SFE_EINVAL               # an odd n_out under TX10
    assert call(n_bursts=2, istride=1 << 62) == L.SFE_EINVAL         # a byte range that reaches 2^62
    assert call(po=d_in.ptr + 8 * ((nb * nbytes - 1) // 8)) == L.SFE_EINVAL      # the output over the payloads
    assert call(pi=out.ptr + 8 * n_out - 1) == L.SFE_EINVAL
    assert call(kk=None) == L.SFE_EINVAL and call(hh=None) == L.SFE_EINVAL
    assert k.value == 0
    # a live handle of another block is refused, and mod's destroy frees nothing of it
    other = api.Corr(np.ones(13, np.complex64), 3840)
    assert call(hh=other._h) == L.SFE_EINVAL and k.value == 0
    assert lib.sfe_dsp_mod_destroy(other._h) == L.SFE_OK
    other.reset()                                                    # still alive
    other.close()
    with pytest.raises(AttributeError):
        h.reset()
    api.sync()
    raw = out.d.to_numpy().view(np.uint32)
    assert (raw == sc.POISON).all()
    # the next good call is a fresh handle's; TX10 output and the payload bytes need no alignment
    assert call() == L.SFE_OK and k.value == n_out
    api.sync()
    assert same(out.take(), api.mod_plan(K, gen, n_info, taps, sps, amp=0.5, data=data, n_out=n_out, start_base=2, start_step=F))
    out.poison()
    assert call(n_bursts=0, pi=None) == L.SFE_OK and k.value == n_out
    api.sync()
    assert not out.take().view(np.uint8).any()
    assert call(n=0, n_bursts=0, po=None, pi=None) == L.SFE_OK and k.value == 0
    outt = Out(api, n_out, True, 3)
    assert call(hh=ht._h, pi=d_in.ptr + 1, istride=nbytes + 1, n_bursts=2, po=outt.ptr) == L.SFE_OK
    api.sync()
    shifted = np.concatenate([data.ravel(), np.zeros(64, np.uint8)])[1:][:2 * (nbytes + 1)].reshape(2, nbytes + 1)
    assert same(outt.take(), api.mod_plan(K, gen, n_info, taps, sps, amp=0.5, out_fmt=L.FMT_TX10, data=shifted, n_out=n_out, start_base=2, start_step=F))
    assert same(h.modulate(data, n_out, 2, F), api.mod_plan(K, gen, n_info, taps, sps, amp=0.5, data=data, n_out=n_out, start_base=2, start_step=F))
    for x in (h, ht):
        x.close()
    for d in (d_in, out, outt):
        d.free()


# ---- behind a decoder, and in front of the receive chain
def test_a_relay_reads_the_decoders_bytes_as_they_lie(api, L):
    """A Vit handle's d_bits and out_stride go straight into Mod: the stream equals the plan's on the decoded bytes."""
    K, gen = K7
    n_info, nb = 106, 5
    want_bits = [synth.vit_bits(n_info, 60 + b) for b in range(nb)]
    soft = np.stack([synth.vit_soft(api.vit_encode(K, gen, bits), 4.0, 0.5, 70 + b) for b, bits in enumerate(want_bits)])
    hv = api.Vit(K, gen, n_info)
    taps = mc.rc_taps(4, 3)
    hm = api.Mod(K, gen, n_info, taps, 4, order=4, amp=0.5)
    F, ostride = hm.frame_len, hv.n_bytes + 3
    n_out = nb * (F + 1) + 9
    d_soft, d_bits = api.DeviceArray.from_numpy(soft), api.DeviceArray.from_bytes(np.full(nb * ostride, 0xEE, np.uint8))
    out = Out(api, n_out, False, 8)
    try:
        assert hv.process_stream(d_soft, nb, d_bits, out_stride=ostride) == nb
        assert hm.process_stream(d_bits, nb, out.ptr, n_out, 3, F + 1, in_stride=ostride) == n_out
        api.sync()
        decoded = d_bits.to_numpy().view(np.uint8)[:nb * ostride].reshape(nb, ostride)
        got = out.take()
    finally:
        for d in (d_soft, d_bits, out):
            d.free()
        hv.close()
        hm.close()
    assert np.array_equal(decoded[:, :hv.n_bytes], np.stack([synth.vit_pack(b) for b in want_bits]))
    assert same(got, api.mod_plan(K, gen, n_info, taps, 4, order=4, amp=0.5, data=decoded, n_out=n_out, start_base=3, start_step=F + 1))


@pytest.mark.parametrize("fmt", ["f32", "tx10-as-u8"])
def test_loopback_returns_the_bytes_that_went_in(api, L, fmt):
    """Mod -> Corr -> Burst -> Vit on the device: the correlator finds every frame where the law puts symbol 0's peak, the
    burst demodulator starts there, and the decoder returns the bytes given to Mod.  With TX10 the receive side reads a
    host-side requantisation of the wire format to (I,Q) bytes: there is no TX10 -> u8 converter on the device."""
    c = mc.CHAIN
    taps, pre, data, tpl = mc.chain_parts()
    nb, n_out = c["n_bursts"], c["n_bursts"] * c["step"]
    u8 = fmt != "f32"
    hm = api.Mod(c["K"], c["gen"], c["n_info"], taps, c["sps"], preamble=pre, amp=c["amp"], out_fmt=L.FMT_TX10 if u8 else L.FMT_F32)
    assert (hm.n_sym, hm.frame_len, hm.n_soft) == (c["N"], c["F"], 224)
    hc = api.Corr(tpl, c["step"], min_energy=c["min_energy"])
    hb = api.Burst(pre, c["sps"], c["N"], c["lag"])
    hv = api.Vit(c["K"], c["gen"], c["n_info"], in_mode=L.VIT_IN_BPSK, skip=c["Lp"])
    if u8:
        hc.set_input_format(L.FMT_U8)
        hb.set_input_format(L.FMT_U8)
    d_data = api.DeviceArray.from_bytes(data)
    out = Out(api, n_out, u8, 0)
    d_val, d_idx = api.DeviceArray(nb), api.DeviceArray(nb)
    d_sym, d_brec, d_bst = api.DeviceArray(nb * c["N"] * 2), api.DeviceArray(nb * 8), api.DeviceArray(nb)
    d_by, d_rec, d_st = api.DeviceArray((nb * hv.n_bytes + 3) // 4), api.DeviceArray(2 * nb), api.DeviceArray(nb)
    held = [d_data, out, d_val, d_idx, d_sym, d_brec, d_bst, d_by, d_rec, d_st]
    try:
        assert hm.process_stream(d_data, nb, out.ptr, n_out, c["base"], c["step"]) == n_out
        x = out.ptr
        if u8:
            api.sync()
            held.append(api.DeviceArray.from_bytes(mc.tx10_as_u8_samples(out.take())))
            x = held[-1].ptr
        assert hc.process_stream(x, n_out, d_val, d_idx) == nb
        assert hb.process_stream(x, n_out, nb, d_sym, d_idx, d_val, d_brec, d_bst, start_base=-(c["tpl_len"] - 1), start_step=c["step"]) == nb
        assert hv.process_stream(d_sym, nb, d_by, d_rec, d_st, d_bst, in_stride=c["N"]) == nb
        api.sync()
        if not u8:
            assert same(out.take(), api.mod_plan(c["K"], c["gen"], c["n_info"], taps, c["sps"], preamble=pre, amp=c["amp"], data=data, n_out=n_out,
                                                 start_base=c["base"], start_step=c["step"]))
        idx, val = d_idx.to_numpy().view(np.uint32), d_val.to_numpy()
        by = d_by.to_numpy().view(np.uint8)[:nb * hv.n_bytes].reshape(nb, hv.n_bytes)
        rec, st, bst = d_rec.to_numpy().view(np.uint32).reshape(nb, 2), d_st.to_numpy().view(np.int32), d_bst.to_numpy().view(np.int32)
    finally:
        for d in held:
            d.free()
        for h in (hm, hc, hb, hv):
            h.close()
    print(fmt, "corr indices", idx, "values", val, "burst statuses", bst, "vit statuses", st, "counts", rec[:, 1])
    assert idx.tolist() == [c["base"] + c["tpl_at"] + c["tpl_len"] - 1] * nb
    assert not bst.any() and not st.any() and not rec[:, 1].any()
    assert np.array_equal(by, data)
