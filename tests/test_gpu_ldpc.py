"""The quasi-cyclic LDPC code (sfe_dsp_ldpc_*) on the GPU.  The bar is equality with api.ldpc_plan -- bytes, record and
status -- never a tolerance: every code and input of tests/ldpc_cases.py at 1, 3 and 67 codewords, both parameter sets, all
three input modes, through the poisoned, guarded layouts of tests/stream_checks.py (payload bases at every byte offset,
strides a few items beyond the row: exactly the call's slots lose their poison and the input is intact afterwards), with
and without the optional buffers; the contracts about bytes checked literally; captured calls replayed onto a poisoned
output; the refusals; and the chain Ldpc.encode_stream -> Mod -> Corr -> Burst -> Ldpc.process_stream on the device."""
import ctypes as C

import numpy as np
import pytest

import ldpc_cases as lc
import stream_checks as sc

pytestmark = pytest.mark.gpu
KEYS = sorted(lc.CASES)


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

    def unwritten(self):
        assert np.array_equal(sc._download(self.d), self.raw)

    def intact(self):
        sc.check_input_intact(sc._download(self.d), self.raw)

    def free(self):
        self.d.free()


def decode(api, h, x, lead=0, in_pad=0, out_lead=0, out_pad=0, rec=True, status=True, status_in=None, call=None):
    """One process_stream through guarded buffers; x: (n_words, row) float32 or complex64 rows of the handle's mode; lead in
    items of the input.  Returns (bytes, record or None, status or None)."""
    nw, item = x.shape[0], x.dtype.itemsize
    b_in = Buf(api, nw, x.shape[1], in_pad, lead * item, item, rows=x)
    b_out = Buf(api, nw, h.k_bytes, out_pad, out_lead)
    b_rec = Buf(api, 1, 3 * nw, item=4) if rec else None
    b_st = Buf(api, 1, nw, item=4) if status else None
    b_si = Buf(api, 1, nw, item=4, rows=[np.asarray(status_in, np.int32)]) if status_in is not None else None
    held = [b for b in (b_in, b_out, b_rec, b_st, b_si) if b is not None]
    try:
        k = (call or h.process_stream)(b_in.ptr, nw, b_out.ptr, b_rec and b_rec.ptr, b_st and b_st.ptr, b_si and b_si.ptr,
                                       in_stride=x.shape[1] + in_pad, out_stride=h.k_bytes + out_pad)
        api.sync()
        assert k == nw
        b_in.intact()
        if b_si:
            b_si.intact()
        return (b_out.written(), b_rec.written(np.uint32).reshape(nw, 3) if rec else None, b_st.written(np.int32).reshape(nw) if status else None)
    finally:
        for b in held:
            b.free()


def encode(api, h, pay, lead=0, in_pad=0, out_lead=0, out_pad=0):
    nw = pay.shape[0]
    b_in = Buf(api, nw, h.k_bytes, in_pad, lead, rows=pay)
    b_out = Buf(api, nw, h.n_bytes, out_pad, out_lead)
    try:
        k = h.encode_stream(b_in.ptr, nw, b_out.ptr, in_stride=h.k_bytes + in_pad, out_stride=h.n_bytes + out_pad)
        api.sync()
        assert k == nw
        b_in.intact()
        return b_out.written()
    finally:
        b_in.free()
        b_out.free()


def same(got, want):
    return all(g is None or (g.dtype == w.dtype and np.array_equal(g, w)) for g, w in zip(got, want))


# (input mode, skip, parameter set) of the four layouts of a call size
LAYOUTS = [(0, 0, "a12"), (1, 3, "a16"), (2, 5, "a12"), (0, 0, "a16")]


@pytest.mark.parametrize("n_words", [1, 3, 67])
@pytest.mark.parametrize("key", KEYS)
def test_decode_and_encode_equal_the_plan(api, L, key, n_words):
    """Four layouts per call size: another input mode, parameter set, input lead and payload base each, strides 1 .. 4 items
    beyond the row; all optional buffers, none, the record alone, status and an upstream table whose words hold only NaNs."""
    s, Z = lc.CASES[key]
    x = lc.many(key, n_words)
    pay = lc.payloads(key, n_words, 11)
    si = (np.arange(n_words) % 5 == 1).astype(np.int32) * 9
    x_si = x.copy()
    x_si[si != 0] = np.nan
    for lead, (mode, skip, pset) in enumerate(LAYOUTS):
        a, beta, max_iter = lc.PARAMS[pset]
        lc.check_the_reference(key, pset)
        opt = [dict(status_in=si), dict(rec=False, status=False), dict(status=False), dict(rec=False, status_in=si)][lead]
        rows = x_si if "status_in" in opt else x
        want = api.ldpc_plan(s, Z, lc.SCALE, a, beta, max_iter, x=rows, status_in=opt.get("status_in"))
        h = api.Ldpc(s, Z, lc.SCALE, a, beta, max_iter, in_mode=mode, skip=skip)
        try:
            assert (h.n, h.k, h.k_bytes, h.n_bytes) == lc.sizes(key) and h.encodable == (key != "G")
            lay = dict(lead=lead, in_pad=1 + lead, out_lead=(3 * lead + 1) % 4, out_pad=4 - lead)
            got = decode(api, h, lc.as_mode(rows, mode, skip), **lay, **opt)
            assert same(got, want), (key, n_words, lead)
            if "status_in" in opt and opt.get("status", True):
                assert (got[2][si != 0] == 2).all() and (want[2][si == 0] != 2).all()
            if key != "G":
                assert np.array_equal(encode(api, h, pay, **lay), api.ldpc_plan(s, Z, data=pay)), (key, n_words, lead)
        finally:
            h.close()


def test_a_code_that_is_not_encodable_decodes_and_refuses_to_encode(api, L):
    s, Z = lc.CASES["G"]
    h = api.Ldpc(s, Z)
    pay = lc.payloads("G", 2, 5)
    b_in, b_out = Buf(api, 2, h.k_bytes, rows=pay), Buf(api, 2, h.n_bytes)
    try:
        assert not h.encodable and api.ldpc_plan(s, Z) == (42, 21, False)
        with pytest.raises(api.SfeError) as e:
            h.encode_stream(b_in.ptr, 2, b_out.ptr)
        assert e.value.code == L.SFE_ESTATE and "ldpc_encode_stream: " in str(e.value)
        api.sync()
        b_out.unwritten()
        x = lc.inputs("G")[1]
        assert same(h.decode(x), lc.reference("G", "a12")[:3])
    finally:
        h.close()
        b_in.free()
        b_out.free()


@pytest.mark.parametrize("key", ["A", "C", "F"])
def test_runs_repeat_and_a_word_depends_on_its_values_alone(api, key):
    """The same call twice; then every word of it alone, as word 0 of a one-word call in another input mode, at another
    address parity and other strides."""
    s, Z = lc.CASES[key]
    names, x = lc.inputs(key)
    nw = x.shape[0]
    pay = lc.payloads(key, nw, 12)
    h = api.Ldpc(s, Z, lc.SCALE, 12, 0, 32)
    hb = api.Ldpc(s, Z, lc.SCALE, 12, 0, 32, in_mode=1, skip=2)
    hq = api.Ldpc(s, Z, lc.SCALE, 12, 0, 32, in_mode=2, skip=1)
    try:
        a = decode(api, h, x, lead=2, in_pad=3, out_lead=1, out_pad=2)
        assert same(decode(api, h, x, lead=2, in_pad=3, out_lead=1, out_pad=2), a) and same(a, lc.reference(key, "a12")[:3])
        ea = encode(api, h, pay, lead=1, in_pad=2, out_lead=3, out_pad=1)
        assert np.array_equal(encode(api, h, pay, lead=1, in_pad=2, out_lead=3, out_pad=1), ea)
        for i in range(nw):
            hh, mode, skip = [(h, 0, 0), (hb, 1, 2), (hq, 2, 1)][i % 3]
            one = decode(api, hh, lc.as_mode(x[i:i + 1], mode, skip), lead=i % 4, in_pad=i % 3, out_lead=(i + 1) % 4, out_pad=i % 5)
            assert same(one, [v[i:i + 1] for v in a]), (i, names[i])
            assert np.array_equal(encode(api, h, pay[i:i + 1], lead=(i + 2) % 4, in_pad=i % 5, out_lead=i % 4, out_pad=i % 3), ea[i:i + 1]), i
    finally:
        for q in (h, hb, hq):
            q.close()


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
    key = "C"
    s, Z = lc.CASES[key]
    x = lc.many(key, 9)
    pay = lc.payloads(key, 9, 13)
    want, want_enc = api.ldpc_plan(s, Z, lc.SCALE, 12, 0, 32, x=x), api.ldpc_plan(s, Z, data=pay)
    h = api.Ldpc(s, Z, lc.SCALE, 12, 0, 32)
    kb, nb, n = h.k_bytes, h.n_bytes, h.n
    b_in, b_pay = Buf(api, 9, n, 3, 4, 4, rows=x), Buf(api, 9, kb, 1, 3, rows=pay)
    b_out, b_rec, b_st, b_enc = Buf(api, 9, kb, 2, 3), Buf(api, 1, 27, item=4), Buf(api, 1, 9, item=4), Buf(api, 9, nb, 2, 1)
    sm, g, ex = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert hip.hipStreamCreate(C.byref(sm)) == 0
    assert hip.hipStreamBeginCapture(sm, 0) == 0
    try:
        k = h.process_stream(b_in.ptr, 9, b_out.ptr, b_rec.ptr, b_st.ptr, in_stride=n + 3, out_stride=kb + 2, stream=sm.value)
        ke = h.encode_stream(b_pay.ptr, 9, b_enc.ptr, in_stride=kb + 1, out_stride=nb + 2, stream=sm.value)
    finally:
        ended = hip.hipStreamEndCapture(sm, C.byref(g))
    assert ended == 0 and k == 9 and ke == 9 and hip.hipGraphInstantiate(C.byref(ex), g, None, None, 0) == 0
    try:
        for _ in range(2):
            for b in (b_out, b_rec, b_st, b_enc):
                b.poison()
            assert hip.hipGraphLaunch(ex, sm) == 0 and hip.hipStreamSynchronize(sm) == 0
            assert same((b_out.written(), b_rec.written(np.uint32).reshape(9, 3), b_st.written(np.int32).reshape(9)), want)
            assert np.array_equal(b_enc.written(), want_enc)
            b_in.intact()
            b_pay.intact()
    finally:
        hip.hipGraphExecDestroy(ex)
        hip.hipGraphDestroy(g)
        hip.hipStreamDestroy(sm)
        h.close()
        for b in (b_in, b_pay, b_out, b_rec, b_st, b_enc):
            b.free()


def test_refusals_launch_nothing(api, L):
    key, nw = "B", 3
    s, Z = lc.CASES[key]
    x = lc.many(key, nw)
    h = api.Ldpc(s, Z, lc.SCALE, 12, 0, 32)
    hq = api.Ldpc(s, Z, lc.SCALE, 12, 0, 32, in_mode=L.VIT_IN_QPSK, skip=4)
    n, kb, nb = h.n, h.k_bytes, h.n_bytes
    assert (n, kb, nb) == (648, 41, 81) and hq.row == 4 + 324
    d_in = api.DeviceArray.from_numpy(np.concatenate([x.ravel(), np.zeros(64, np.float32)]))
    poison = np.full(256, sc.POISON, np.uint32)
    d_out, d_rec, d_st, d_si = (sc._upload(api, poison) for _ in range(4))
    d_si.zero()
    lib = L.load()
    k = C.c_size_t(7)

    def call(pi=d_in.ptr, istride=n, psi=d_si.ptr, nn=nw, po=d_out.ptr, ostride=kb, pr=d_rec.ptr, ps=d_st.ptr, hh=None, kk=C.byref(k)):
        return lib.sfe_dsp_ldpc_process_stream(hh or h._h, pi, istride, psi, nn, po, ostride, pr, ps, kk, None)

    def enc(pi=d_in.ptr, istride=kb, nn=nw, po=d_out.ptr, ostride=nb, hh=None, kk=C.byref(k)):
        return lib.sfe_dsp_ldpc_encode_stream(hh or h._h, pi, istride, nn, po, ostride, kk, None)

    assert call(istride=n - 1) == L.SFE_ERANGE and lib.sfe_dsp_last_error().startswith(b"ldpc_process_stream: ")
    assert call(ostride=kb - 1) == L.SFE_ERANGE
    assert call(hh=hq._h, istride=hq.row - 1) == L.SFE_ERANGE and call(hh=hq._h, istride=hq.row, nn=1) == L.SFE_OK       # skip + ceil(n / 2) symbols
    api.sync()
    for d in (d_out, d_rec, d_st):                                  # that one good call wrote: poison again
        api.check(lib.sfe_dsp_memcpy_h2d(d.ptr, poison.ctypes.data, poison.nbytes, None))
    api.sync()
    k.value = 7
    assert enc(istride=kb - 1) == L.SFE_ERANGE and lib.sfe_dsp_last_error().startswith(b"ldpc_encode_stream: ")
    assert enc(ostride=nb - 1) == L.SFE_ERANGE
    assert call(pi=None) == L.SFE_EINVAL and call(po=None) == L.SFE_EINVAL and enc(pi=None) == L.SFE_EINVAL and enc(po=None) == L.SFE_EINVAL
    assert call(pi=d_in.ptr + 2) == L.SFE_EINVAL                     # misaligned: soft values, symbols, each four-byte table
    assert call(hh=hq._h, pi=d_in.ptr + 4, istride=hq.row) == L.SFE_EINVAL
    assert call(psi=d_si.ptr + 1) == L.SFE_EINVAL
    assert call(pr=d_rec.ptr + 2) == L.SFE_EINVAL
    assert call(ps=d_st.ptr + 3) == L.SFE_EINVAL
    assert call(nn=1 << 31) == L.SFE_EINVAL and enc(nn=1 << 31) == L.SFE_EINVAL
    assert call(istride=1 << 62) == L.SFE_EINVAL and call(ostride=1 << 62) == L.SFE_EINVAL       # byte ranges that reach 2^62
    assert enc(istride=1 << 62) == L.SFE_EINVAL and enc(ostride=1 << 62) == L.SFE_EINVAL
    assert call(po=d_in.ptr + 4 * nw * n - 1) == L.SFE_EINVAL        # each output over the input and over the status table
    assert call(pr=d_in.ptr) == L.SFE_EINVAL and call(ps=d_in.ptr + 8) == L.SFE_EINVAL
    assert call(po=d_si.ptr + 4 * nw - 1) == L.SFE_EINVAL and call(pr=d_si.ptr + 4) == L.SFE_EINVAL and call(ps=d_si.ptr) == L.SFE_EINVAL
    assert call(pr=d_out.ptr + 8) == L.SFE_EINVAL                    # two outputs over one another
    assert call(ps=d_out.ptr + 4 * ((nw * kb - 1) // 4)) == L.SFE_EINVAL
    assert call(ps=d_rec.ptr + 4) == L.SFE_EINVAL
    assert enc(po=d_in.ptr + nw * kb - 1) == L.SFE_EINVAL and enc(pi=d_out.ptr + nw * nb - 1) == L.SFE_EINVAL
    assert call(kk=None) == L.SFE_EINVAL and enc(kk=None) == L.SFE_EINVAL
    assert k.value == 0
    assert call(nn=0) == L.SFE_OK and k.value == 0 and enc(nn=0) == L.SFE_OK and k.value == 0      # no codewords: a no-op
    # a live handle of another block is refused, and ldpc's destroy frees nothing of it
    other = api.Corr(np.ones(13, np.complex64), 3840)
    assert call(hh=other._h) == L.SFE_EINVAL and enc(hh=other._h) == L.SFE_EINVAL and k.value == 0
    assert lib.sfe_dsp_ldpc_destroy(other._h) == L.SFE_OK
    other.reset()                                                    # still alive
    other.close()
    with pytest.raises(AttributeError):
        h.reset()
    api.sync()
    for d in (d_out, d_rec, d_st):
        assert np.array_equal(sc._download(d), poison)
    # the next good call is a fresh handle's; the optional buffers may be left out
    want = api.ldpc_plan(s, Z, lc.SCALE, 12, 0, 32, x=x)
    assert call() == L.SFE_OK and k.value == nw
    assert call(psi=None, pr=None, ps=None) == L.SFE_OK and k.value == nw
    api.sync()
    assert np.array_equal(d_out.to_numpy().view(np.uint8)[:nw * kb].reshape(nw, kb), want[0])
    assert np.array_equal(d_rec.to_numpy(3 * nw).view(np.uint32).reshape(nw, 3), want[1])
    assert np.array_equal(d_st.to_numpy(nw).view(np.int32), want[2])
    assert same(h.decode(x), want)
    assert np.array_equal(h.encode(want[0]), api.ldpc_plan(s, Z, data=want[0]))
    h.close()
    hq.close()
    for d in (d_in, d_out, d_rec, d_st, d_si):
        d.free()


def test_the_chain_stays_on_the_device(api, L):
    """Ldpc.encode_stream -> Mod (uncoded, QPSK, a preamble) -> Corr -> Burst -> Ldpc.process_stream (QPSK input, skip = Lp,
    the burst demodulator's status table): only handles, pointers and strides pass between the blocks.  Between Mod and
    Corr a stretch of burst 1's waveform is negated -- chosen on the CPU, through the host plans, so that the decoder has
    wrong decisions to repair.  The payloads come back, burst 1's record counts the repairs, and every status is 0."""
    c, key = lc.LINK, lc.LINK_KEY
    s, Z = lc.CASES[key]
    a_, beta, max_iter = lc.LINK_PARAMS
    taps, pre, tpl, pay = lc.link_parts()
    (a, b), code, cpu_dec = lc.link_on_the_cpu(api, L)
    nb, n_out = c["n_bursts"], c["n_bursts"] * c["step"]
    he = api.Ldpc(s, Z)
    hd = api.Ldpc(s, Z, lc.SCALE, a_, beta, max_iter, in_mode=L.VIT_IN_QPSK, skip=c["Lp"])
    hm = api.Mod(0, None, c["n_info"], taps, c["sps"], order=4, preamble=pre, amp=c["amp"])
    assert (he.k_bytes, he.n_bytes, hm.n_bytes, hm.n_sym, hm.frame_len, hd.row) == (41, 81, 81, c["N"], c["F"], c["N"])
    hc = api.Corr(tpl, c["step"], min_energy=c["min_energy"])
    hb = api.Burst(pre, c["sps"], c["N"], c["lag"])
    d_pay, d_code, d_x = api.DeviceArray.from_bytes(pay), api.DeviceArray(nb * 81 // 4 + 4), api.DeviceArray(2 * n_out)
    d_val, d_idx = api.DeviceArray(nb), api.DeviceArray(nb)
    d_sym, d_brec, d_bst = api.DeviceArray(nb * c["N"] * 2), api.DeviceArray(nb * 8), api.DeviceArray(nb)
    d_out, d_rec, d_st = api.DeviceArray(nb * 41 // 4 + 4), api.DeviceArray(3 * nb), api.DeviceArray(nb)
    held = [d_pay, d_code, d_x, d_val, d_idx, d_sym, d_brec, d_bst, d_out, d_rec, d_st]
    try:
        assert he.encode_stream(d_pay, nb, d_code) == nb
        assert hm.process_stream(d_code, nb, d_x, n_out, c["base"], c["step"], in_stride=81) == n_out
        api.sync()
        part = -d_x.to_numpy(2 * (b - a), offset=2 * a)             # the channel: a stretch of the waveform negated
        api.check(d_x._L.sfe_dsp_memcpy_h2d(d_x.ptr + 8 * a, part.ctypes.data, part.nbytes, None))
        api.sync()
        assert hc.process_stream(d_x, n_out, d_val, d_idx) == nb
        assert hb.process_stream(d_x, n_out, nb, d_sym, d_idx, d_val, d_brec, d_bst, start_base=-(c["tpl_len"] - 1), start_step=c["step"]) == nb
        assert hd.process_stream(d_sym, nb, d_out, d_rec, d_st, d_bst, in_stride=c["N"]) == nb
        api.sync()
        sent = d_code.to_numpy().view(np.uint8)[:nb * 81].reshape(nb, 81)
        out = d_out.to_numpy().view(np.uint8)[:nb * 41].reshape(nb, 41)
        rec, st = d_rec.to_numpy(3 * nb).view(np.uint32).reshape(nb, 3), d_st.to_numpy().view(np.int32)
        bst, idx = d_bst.to_numpy().view(np.int32), d_idx.to_numpy().view(np.uint32)
    finally:
        for d in held:
            d.free()
        for h in (he, hd, hm, hc, hb):
            h.close()
    print("corr indices", idx, "burst statuses", bst, "records", rec.tolist(), "statuses", st)
    assert np.array_equal(sent, code) and idx.tolist() == [c["base"] + c["tpl_at"] + c["tpl_len"] - 1] * nb
    assert not bst.any() and not st.any()
    assert np.array_equal(out, lc.payload_bits_only(key, pay)) and rec[1, 0] >= 1 and rec[1, 2] >= 2 and not rec[:, 1].any()
    assert same((out, rec, st), cpu_dec)
