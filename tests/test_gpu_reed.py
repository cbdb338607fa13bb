"""The Reed-Solomon outer code (sfe_dsp_reed_*) on the GPU.  The bar is equality with api.reed_plan -- bytes, record and
status -- never a tolerance: every shape and error pattern of tests/reed_cases.py at 1, 3 and 257 frames, through the
poisoned, guarded layouts of tests/stream_checks.py (input leads of 0 .. 3 bytes, strides a few bytes beyond the row:
exactly the call's slots lose their poison and the input is intact afterwards), with and without the optional buffers;
the contracts about bytes checked literally; captured calls replayed onto a poisoned output; the refusals; and the chain
Reed.encode_stream -> Mod -> Corr -> Burst -> Vit -> Reed.process_stream on the device."""
import ctypes as C

import numpy as np
import pytest

import reed_cases as rc
import stream_checks as sc

pytestmark = pytest.mark.gpu
F32 = np.float32
KEYS = sorted(rc.SHAPES)


@pytest.fixture(scope="module")
def api():
    from simplefe_amd import api as a
    return a


@pytest.fixture(scope="module")
def L():
    from simplefe_amd import lib
    return lib


class Buf:
    """n_rows rows of `row` items of `item` bytes on the device, `pad` items apart, `lead` bytes behind a 64-byte front
    guard, poison everywhere else (stream_checks' layout and poison)."""

    def __init__(self, api, n_rows, row, pad=0, lead=0, item=1, rows=None):
        self.api, self.k = api, row
        self.lay = sc.Layout(n_rows, item, row, row + pad, 64 + lead, 64, 4)
        self.raw = self.lay.poisoned()
        if rows is not None:
            for c in range(n_rows):
                self.lay.put(self.raw, c, rows[c])
        self.d = sc._upload(api, self.raw)
        self.ptr = self.d.ptr + self.lay.front

    def poison(self):
        self.api.check(self.d._L.sfe_dsp_memcpy_h2d(self.d.ptr, self.raw.ctypes.data, self.raw.nbytes, None))
        self.api.sync()

    def written(self, dtype=np.uint8):
        """The rows, after checking that every cell of them was stored and not a byte outside them."""
        raw = sc._download(self.d)
        sc.check_written(raw, self.lay, self.k)
        return np.stack([self.lay.take(raw, c, self.k, dtype) for c in range(self.lay.n_channels)])

    def intact(self):
        sc.check_input_intact(sc._download(self.d), self.raw)

    def free(self):
        self.d.free()


def decode(api, h, frames, lead=0, in_pad=0, out_lead=0, out_pad=0, rec=True, status=True, status_in=None, call=None):
    """One process_stream through guarded buffers; returns (bytes, record or None, status or None)."""
    nf = frames.shape[0]
    b_in = Buf(api, nf, h.frame_bytes, in_pad, lead, rows=frames)
    b_out = Buf(api, nf, h.payload_bytes, out_pad, out_lead)
    b_rec = Buf(api, 1, 2 * nf, item=4) if rec else None
    b_st = Buf(api, 1, nf, item=4) if status else None
    b_si = Buf(api, 1, nf, item=4, rows=[np.asarray(status_in, np.int32)]) if status_in is not None else None
    held = [b for b in (b_in, b_out, b_rec, b_st, b_si) if b is not None]
    try:
        k = (call or h.process_stream)(b_in.ptr, nf, b_out.ptr, b_rec and b_rec.ptr, b_st and b_st.ptr, b_si and b_si.ptr,
                                       in_stride=h.frame_bytes + in_pad, out_stride=h.payload_bytes + out_pad)
        api.sync()
        assert k == nf
        b_in.intact()
        if b_si:
            b_si.intact()
        return (b_out.written(), b_rec.written(np.uint32).reshape(nf, 2) if rec else None, b_st.written(np.int32).reshape(nf) if status else None)
    finally:
        for b in held:
            b.free()


def encode(api, h, pay, lead=0, in_pad=0, out_lead=0, out_pad=0, call=None):
    nf = pay.shape[0]
    b_in = Buf(api, nf, h.payload_bytes, in_pad, lead, rows=pay)
    b_out = Buf(api, nf, h.frame_bytes, out_pad, out_lead)
    try:
        k = (call or h.encode_stream)(b_in.ptr, nf, b_out.ptr, in_stride=h.payload_bytes + in_pad, out_stride=h.frame_bytes + out_pad)
        api.sync()
        assert k == nf
        b_in.intact()
        return b_out.written()
    finally:
        b_in.free()
        b_out.free()


def same(got, want):
    return all(g is None or (g.dtype == w.dtype and np.array_equal(g, w)) for g, w in zip(got, want))


@pytest.mark.parametrize("n_frames", [1, 3, 257])
@pytest.mark.parametrize("key", KEYS)
def test_decode_and_encode_equal_the_plan(api, key, n_frames):
    """Four layouts per call size: input leads of 0 .. 3 bytes, outputs at other byte offsets, strides 1 .. 4 bytes beyond
    the row; all optional buffers, none, the record alone, status and an upstream table."""
    shape = rc.SHAPES[key]
    rc.check_the_reference(key)
    frames, wh = rc.many(key, n_frames)
    pay = rc.payloads(shape, n_frames, 11)
    si = (np.arange(n_frames) % 5 == 1).astype(np.int32) * 9
    want, want_si = api.reed_plan(*shape, whiten=wh, data=frames), api.reed_plan(*shape, whiten=wh, data=frames, status_in=si)
    want_enc = api.reed_plan(*shape, whiten=wh, data=pay, encode=True)
    if n_frames == rc.patterns(key)[2].shape[0]:
        assert same(want, rc.reference(key))
    h = api.Reed(*shape, whiten=wh)
    try:
        assert (h.payload_bytes, h.frame_bytes, h.t) == rc.sizes(shape)
        for lead in range(4):
            lay = dict(lead=lead, in_pad=1 + lead, out_lead=(3 * lead + 1) % 4, out_pad=4 - lead)
            opt = [dict(status_in=si), dict(rec=False, status=False), dict(status=False), dict(rec=False, status_in=si)][lead]
            got = decode(api, h, frames, **lay, **opt)
            assert same(got, want_si if "status_in" in opt else want), (key, n_frames, lead)
            assert np.array_equal(encode(api, h, pay, **lay), want_enc), (key, n_frames, lead)
    finally:
        h.close()


def test_no_whitening_is_no_table(api):
    """A handle made without a sequence: the plan's bytes without one, both ways."""
    shape = rc.SHAPES["C"]
    names, pay, frames, _ = rc.patterns("C", False)
    h = api.Reed(*shape)
    try:
        assert same(decode(api, h, frames, lead=1, in_pad=2, out_lead=3, out_pad=1), api.reed_plan(*shape, data=frames))
        assert np.array_equal(encode(api, h, pay, lead=3, in_pad=1, out_lead=2, out_pad=3), api.reed_plan(*shape, data=pay, encode=True))
    finally:
        h.close()


@pytest.mark.parametrize("key", ["A", "C", "D"])
def test_runs_repeat_and_a_frame_depends_on_its_bytes_alone(api, key):
    """The same call twice; then every frame of it alone, as frame 0 of a one-frame call at another address parity and
    other strides."""
    shape = rc.SHAPES[key]
    nf = rc.patterns(key)[2].shape[0]
    frames, wh = rc.many(key, nf)
    pay = rc.payloads(shape, nf, 12)
    h = api.Reed(*shape, whiten=wh)
    try:
        a = decode(api, h, frames, lead=2, in_pad=3, out_lead=1, out_pad=2)
        assert same(decode(api, h, frames, lead=2, in_pad=3, out_lead=1, out_pad=2), a) and same(a, api.reed_plan(*shape, whiten=wh, data=frames))
        ea = encode(api, h, pay, lead=1, in_pad=2, out_lead=3, out_pad=1)
        assert np.array_equal(encode(api, h, pay, lead=1, in_pad=2, out_lead=3, out_pad=1), ea)
        for i in range(nf):
            one = decode(api, h, frames[i:i + 1], lead=i % 4, in_pad=i % 3, out_lead=(i + 1) % 4, out_pad=i % 5)
            assert same(one, [v[i:i + 1] for v in a]), i
            assert np.array_equal(encode(api, h, pay[i:i + 1], lead=(i + 2) % 4, in_pad=i % 5, out_lead=i % 4, out_pad=i % 3), ea[i:i + 1]), i
    finally:
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


def test_captured_calls_replay_onto_a_poisoned_output(api):
    """Nothing in a handle changes after create, so both calls are supported under graph capture: the two nodes -- a decode
    and an encode -- are replayed twice, the outputs poisoned again in between, and both times the bytes equal the plan's."""
    hip = hip_runtime()
    shape = rc.SHAPES["C"]
    frames, wh = rc.many("C", 9)
    pay = rc.payloads(shape, 9, 13)
    want, want_enc = api.reed_plan(*shape, whiten=wh, data=frames), api.reed_plan(*shape, whiten=wh, data=pay, encode=True)
    h = api.Reed(*shape, whiten=wh)
    P, Fb = h.payload_bytes, h.frame_bytes
    b_in, b_pay = Buf(api, 9, Fb, 3, 1, rows=frames), Buf(api, 9, P, 1, 3, rows=pay)
    b_out, b_rec, b_st, b_enc = Buf(api, 9, P, 2, 3), Buf(api, 1, 18, item=4), Buf(api, 1, 9, item=4), Buf(api, 9, Fb, 2, 1)
    s, g, ex = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert hip.hipStreamCreate(C.byref(s)) == 0
    assert hip.hipStreamBeginCapture(s, 0) == 0
    try:
        k = h.process_stream(b_in.ptr, 9, b_out.ptr, b_rec.ptr, b_st.ptr, in_stride=Fb + 3, out_stride=P + 2, stream=s.value)
        ke = h.encode_stream(b_pay.ptr, 9, b_enc.ptr, in_stride=P + 1, out_stride=Fb + 2, stream=s.value)
    finally:
        ended = hip.hipStreamEndCapture(s, C.byref(g))
    assert ended == 0 and k == 9 and ke == 9 and hip.hipGraphInstantiate(C.byref(ex), g, None, None, 0) == 0
    try:
        for _ in range(2):
            for b in (b_out, b_rec, b_st, b_enc):
                b.poison()
            assert hip.hipGraphLaunch(ex, s) == 0 and hip.hipStreamSynchronize(s) == 0
            assert same((b_out.written(), b_rec.written(np.uint32).reshape(9, 2), b_st.written(np.int32).reshape(9)), want)
            assert np.array_equal(b_enc.written(), want_enc)
            b_in.intact()
            b_pay.intact()
    finally:
        hip.hipGraphExecDestroy(ex)
        hip.hipGraphDestroy(g)
        hip.hipStreamDestroy(s)
        h.close()
        for b in (b_in, b_pay, b_out, b_rec, b_st, b_enc):
            b.free()


def test_refusals_launch_nothing(api, L):
    shape = rc.SHAPES["C"]
    nf = 3
    frames, wh = rc.many("C", nf)
    h = api.Reed(*shape, whiten=wh)
    P, Fb = h.payload_bytes, h.frame_bytes
    assert (P, Fb) == (96, 120)
    d_in = api.DeviceArray.from_bytes(np.concatenate([frames.ravel(), np.zeros(64, np.uint8)]))
    poison = np.full(256, sc.POISON, np.uint32)
    d_out, d_rec, d_st, d_si = (sc._upload(api, poison) for _ in range(4))
    d_si.zero()
    lib = L.load()
    k = C.c_size_t(7)

    def call(pi=d_in.ptr, istride=Fb, psi=d_si.ptr, n=nf, po=d_out.ptr, ostride=P, pr=d_rec.ptr, ps=d_st.ptr, hh=None, kk=C.byref(k)):
        return lib.sfe_dsp_reed_process_stream(hh or h._h, pi, istride, psi, n, po, ostride, pr, ps, kk, None)

    def enc(pi=d_in.ptr, istride=P, n=nf, po=d_out.ptr, ostride=Fb, hh=None, kk=C.byref(k)):
        return lib.sfe_dsp_reed_encode_stream(hh or h._h, pi, istride, n, po, ostride, kk, None)

    assert call(istride=Fb - 1) == L.SFE_ERANGE and lib.sfe_dsp_last_error().startswith(b"reed_process_stream: ")
    assert call(ostride=P - 1) == L.SFE_ERANGE
    assert enc(istride=P - 1) == L.SFE_ERANGE and lib.sfe_dsp_last_error().startswith(b"reed_encode_stream: ")
    assert enc(ostride=Fb - 1) == L.SFE_ERANGE
    assert call(pi=None) == L.SFE_EINVAL and call(po=None) == L.SFE_EINVAL and enc(pi=None) == L.SFE_EINVAL and enc(po=None) == L.SFE_EINVAL
    assert call(psi=d_si.ptr + 1) == L.SFE_EINVAL                    # misaligned, each of the four-byte buffers
    assert call(pr=d_rec.ptr + 2) == L.SFE_EINVAL
    assert call(ps=d_st.ptr + 3) == L.SFE_EINVAL
    assert call(n=1 << 31) == L.SFE_EINVAL and enc(n=1 << 31) == L.SFE_EINVAL
    assert call(istride=1 << 62) == L.SFE_EINVAL and call(ostride=1 << 62) == L.SFE_EINVAL       # byte ranges that reach 2^62
    assert enc(istride=1 << 62) == L.SFE_EINVAL and enc(ostride=1 << 62) == L.SFE_EINVAL
    assert call(po=d_in.ptr + nf * Fb - 1) == L.SFE_EINVAL           # each output over the input and over the status table
    assert call(pr=d_in.ptr) == L.SFE_EINVAL and call(ps=d_in.ptr + 8) == L.SFE_EINVAL
    assert call(po=d_si.ptr + 4 * nf - 1) == L.SFE_EINVAL and call(pr=d_si.ptr + 4) == L.SFE_EINVAL and call(ps=d_si.ptr) == L.SFE_EINVAL
    assert call(pr=d_out.ptr + 8) == L.SFE_EINVAL                    # two outputs over one another
    assert call(ps=d_out.ptr + 4 * ((nf * P - 1) // 4)) == L.SFE_EINVAL
    assert call(ps=d_rec.ptr + 4) == L.SFE_EINVAL
    assert enc(po=d_in.ptr + nf * P - 1) == L.SFE_EINVAL and enc(pi=d_out.ptr + nf * Fb - 1) == L.SFE_EINVAL
    assert call(kk=None) == L.SFE_EINVAL and enc(kk=None) == L.SFE_EINVAL
    assert k.value == 0
    assert call(n=0) == L.SFE_OK and k.value == 0 and enc(n=0) == L.SFE_OK and k.value == 0      # no frames: a no-op
    # a live handle of another block is refused, and reed's destroy frees nothing of it
    other = api.Corr(np.ones(13, np.complex64), 3840)
    assert call(hh=other._h) == L.SFE_EINVAL and enc(hh=other._h) == L.SFE_EINVAL and k.value == 0
    assert lib.sfe_dsp_reed_destroy(other._h) == L.SFE_OK
    other.reset()                                                    # still alive
    other.close()
    with pytest.raises(AttributeError):
        h.reset()
    api.sync()
    for d in (d_out, d_rec, d_st):
        assert np.array_equal(sc._download(d), poison)
    # the next good call is a fresh handle's; the optional buffers may be left out
    want = api.reed_plan(*shape, whiten=wh, data=frames)
    assert call() == L.SFE_OK and k.value == nf
    assert call(psi=None, pr=None, ps=None) == L.SFE_OK and k.value == nf
    api.sync()
    assert np.array_equal(d_out.to_numpy().view(np.uint8)[:nf * P].reshape(nf, P), want[0])
    assert np.array_equal(d_rec.to_numpy(2 * nf).view(np.uint32).reshape(nf, 2), want[1])
    assert np.array_equal(d_st.to_numpy(nf).view(np.int32), want[2])
    assert same(h.decode(frames), want)
    assert np.array_equal(h.encode(want[0]), api.reed_plan(*shape, whiten=wh, data=want[0], encode=True))
    h.close()
    for d in (d_in, d_out, d_rec, d_st, d_si):
        d.free()


def test_the_chain_stays_on_the_device(api, L):
    """Reed.encode_stream -> Mod -> Corr -> Burst -> Vit -> Reed.process_stream: only handles, pointers and strides pass
    between the blocks.  Between Mod and Corr a stretch of frame 1's waveform is negated -- chosen on the CPU, through
    the host plans, so that the inner decoder's bytes for that frame are wrong and no codeword holds more than t of them.
    The payloads come back, frame 1's record counts the repairs, and every status is 0."""
    c, code = rc.LINK, rc.LINK_CODE
    taps, pre, tpl, pay, wh = rc.link_parts()
    (a, b), frames, cpu_by, cpu_dec = rc.link_on_the_cpu(api, L)
    assert not np.array_equal(cpu_by[1], frames[1]) and np.array_equal(cpu_by[[0, 2]], frames[[0, 2]])
    assert np.array_equal(cpu_dec[0], pay) and cpu_dec[1][1, 0] >= 1 and not cpu_dec[1][:, 1].any() and not cpu_dec[2].any()
    nb, n_out = c["n_bursts"], c["n_bursts"] * c["step"]
    hr = api.Reed(*code, whiten=wh)
    hm = api.Mod(c["K"], c["gen"], c["n_info"], taps, c["sps"], preamble=pre, amp=c["amp"])
    assert (hr.payload_bytes, hr.frame_bytes, hm.n_bytes, hm.n_sym, hm.frame_len) == (24, 40, 40, c["N"], c["F"])
    hc = api.Corr(tpl, c["step"], min_energy=c["min_energy"])
    hb = api.Burst(pre, c["sps"], c["N"], c["lag"])
    hv = api.Vit(c["K"], c["gen"], c["n_info"], in_mode=L.VIT_IN_BPSK, skip=c["Lp"])
    Fb = hr.frame_bytes
    d_pay, d_frm, d_x = api.DeviceArray.from_bytes(pay), api.DeviceArray(nb * Fb // 4 + 4), api.DeviceArray(2 * n_out)
    d_val, d_idx = api.DeviceArray(nb), api.DeviceArray(nb)
    d_sym, d_brec, d_bst = api.DeviceArray(nb * c["N"] * 2), api.DeviceArray(nb * 8), api.DeviceArray(nb)
    d_by, d_vrec, d_vst = api.DeviceArray(nb * Fb // 4 + 4), api.DeviceArray(2 * nb), api.DeviceArray(nb)
    d_out, d_rec, d_st = api.DeviceArray(nb * 24 // 4 + 4), api.DeviceArray(2 * nb), api.DeviceArray(nb)
    held = [d_pay, d_frm, d_x, d_val, d_idx, d_sym, d_brec, d_bst, d_by, d_vrec, d_vst, d_out, d_rec, d_st]
    try:
        assert hr.encode_stream(d_pay, nb, d_frm) == nb
        assert hm.process_stream(d_frm, nb, d_x, n_out, c["base"], c["step"], in_stride=Fb) == n_out
        api.sync()
        part = -d_x.to_numpy(2 * (b - a), offset=2 * a)             # the channel: a stretch of the waveform negated
        api.check(d_x._L.sfe_dsp_memcpy_h2d(d_x.ptr + 8 * a, part.ctypes.data, part.nbytes, None))
        api.sync()
        assert hc.process_stream(d_x, n_out, d_val, d_idx) == nb
        assert hb.process_stream(d_x, n_out, nb, d_sym, d_idx, d_val, d_brec, d_bst, start_base=-(c["tpl_len"] - 1), start_step=c["step"]) == nb
        assert hv.process_stream(d_sym, nb, d_by, d_vrec, d_vst, d_bst, in_stride=c["N"], out_stride=Fb) == nb
        assert hr.process_stream(d_by, nb, d_out, d_rec, d_st, d_vst, in_stride=Fb) == nb
        api.sync()
        sent = d_frm.to_numpy().view(np.uint8)[:nb * Fb].reshape(nb, Fb)
        by = d_by.to_numpy().view(np.uint8)[:nb * Fb].reshape(nb, Fb)
        out = d_out.to_numpy().view(np.uint8)[:nb * 24].reshape(nb, 24)
        rec, st = d_rec.to_numpy().view(np.uint32).reshape(nb, 2), d_st.to_numpy().view(np.int32)
        vst, bst, idx = d_vst.to_numpy().view(np.int32), d_bst.to_numpy().view(np.int32), d_idx.to_numpy().view(np.uint32)
    finally:
        for d in held:
            d.free()
        for h in (hr, hm, hc, hb, hv):
            h.close()
    print("corr indices", idx, "burst statuses", bst, "vit statuses", vst, "wrong vit bytes", (by != sent).sum(axis=1), "records", rec.tolist(), "statuses", st)
    assert np.array_equal(sent, frames) and idx.tolist() == [c["base"] + c["tpl_at"] + c["tpl_len"] - 1] * nb
    assert not bst.any() and not vst.any() and not st.any()
    assert not np.array_equal(by[1], sent[1]) and np.array_equal(by[[0, 2]], sent[[0, 2]])
    assert np.array_equal(out, pay) and rec[1, 0] >= 1 and not rec[:, 1].any()
    assert same((out, rec, st), api.reed_plan(*code, whiten=wh, data=by, status_in=vst))
