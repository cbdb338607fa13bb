"""The frame check (sfe_dsp_crc_*) on the GPU.  The bar is equality with api.crc_plan -- bytes, record and status -- never a
tolerance: every catalogue model, scrambler-only handles and each sequence of tests/crc_cases.py over payload lengths on
both sides of every boundary of the kernels as built, at 1, 3 and 257 frames, through the poisoned, guarded layouts of
tests/stream_checks.py (input leads of 0 .. 3 bytes, strides a few bytes beyond the row: exactly the call's slots lose their
poison and the input is intact afterwards), with and without the optional buffers; the record against zlib and binascii
directly; more frames than one row of the grid; the contracts about bytes checked literally; captured calls replayed onto
a poisoned output; the refusals; and the chain Crc.append -> Reed.encode -> channel -> Reed.process -> Crc.check on the
device, where the CRC catches the miscorrection the outer code cannot see."""
import binascii
import ctypes as C
import zlib

import numpy as np
import pytest

import crc_cases as cc
import stream_checks as sc

pytestmark = pytest.mark.gpu

# The kernels' boundaries (simplefe_amd/csrc/crc.h), and the payload lengths on both sides of each:
SHORT_MAX = 4096        # CRC_SHORT_MAX: payloads up to this take the wave-per-frame class, longer ones a workgroup per frame
SHORT_ROUND = 4 * 64    # a round of the short class: CRC_SHORT_T = 64 lanes, a dword each; a piece is 4 bytes
LONG_ROUND = 4 * 1024   # a round of the long class: CRC_LONG_T = 1024 lanes
ISSUE_LENGTHS = (1, 3, 4, 5, 15, 16, 17, 1019, 1020, 1021, 1023, 1024, 1025, 4099, 65541, 1 << 20)
BOUNDARY_LENGTHS = (7, 8, 9,                                                    # the second piece
                    SHORT_ROUND - 1, SHORT_ROUND, SHORT_ROUND + 1, SHORT_ROUND + 4, 2 * SHORT_ROUND - 1, 2 * SHORT_ROUND, 2 * SHORT_ROUND + 1,
                    SHORT_MAX - 1, SHORT_MAX, SHORT_MAX + 1, SHORT_MAX + 4,       # the last short rows, the first long ones
                    2 * LONG_ROUND - 1, 2 * LONG_ROUND, 2 * LONG_ROUND + 1)       # the long class's second round
LENGTHS = tuple(sorted(set(ISSUE_LENGTHS + BOUNDARY_LENGTHS)))
LARGEST = LENGTHS[-2:]                                                          # 65 541 and 2^20: three frames only
GRID_X = 1 << 20        # CRC_GRID_X_LOG2 (crc.hip): groups in a row of the grid; a short group is CRC_SHORT_FPB = 4 frames

# every catalogue model, the sequences dealt over them in turn; then each sequence alone (width 0)
PNS = ((0, 0, 0), cc.PN_CCSDS, cc.PN_80211, cc.PN_LONG)
HANDLES = {name: (*cc.model(name), *PNS[i % 4]) for i, name in enumerate(cc.NAMES)}
HANDLES.update({"scrambler/CCSDS": (0, 0, 0, 0, 0, *cc.PN_CCSDS), "scrambler/802.11": (0, 0, 0, 0, 0, *cc.PN_80211),
                "scrambler/32": (0, 0, 0, 0, 0, *cc.PN_LONG)})


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
    guard, poison everywhere else (stream_checks' layout and poison).  Up to MANY rows the verdict on what was written is
    stream_checks.check_written's; beyond, where its loop over the rows would take minutes, the same two facts are read off
    whole arrays: not a byte outside the rows lost its poison, and the rows are returned to be compared with the plan's."""
    MANY = 4096

    def __init__(self, api, n_rows, row, pad=0, lead=0, item=1, rows=None):
        self.api, self.k = api, row
        self.lay = sc.Layout(n_rows, item, row, row + pad, 64 + lead, 64, 4)
        self.raw = self.lay.poisoned()
        if rows is not None:
            self.body(self.raw)[:, :self.lay.cap] = np.ascontiguousarray(rows).view(np.uint8).reshape(n_rows, self.lay.cap)
        self.d = sc._upload(api, self.raw)
        self.ptr = self.d.ptr + self.lay.front

    def body(self, raw):
        """The rows with the gaps behind them, (n_rows, stride) bytes (the tail guard covers the last row's gap)."""
        n, stride = self.lay.n_channels, self.lay.stride
        return raw.view(np.uint8)[self.lay.front:self.lay.front + n * stride].reshape(n, stride)

    def poison(self):
        self.api.check(self.d._L.sfe_dsp_memcpy_h2d(self.d.ptr, self.raw.ctypes.data, self.raw.nbytes, None))
        self.api.sync()

    def written(self, dtype=np.uint8):
        """The rows, after checking that every cell of them was stored and not a byte outside them."""
        raw = sc._download(self.d)
        if self.lay.n_channels <= self.MANY:
            sc.check_written(raw, self.lay, self.k)
        else:
            kept = raw.view(np.uint8) == self.lay.poisoned().view(np.uint8)
            self.body(kept)[:, :self.lay.cap] = True
            assert kept.all(), "a store outside the rows: byte %d" % int(np.flatnonzero(~kept)[0])
        return np.ascontiguousarray(self.body(raw)[:, :self.lay.cap]).view(dtype)

    def untouched(self):
        assert np.array_equal(sc._download(self.d), self.raw)

    def intact(self):
        sc.check_input_intact(sc._download(self.d), self.raw)

    def free(self):
        self.d.free()


def check(api, h, frames, lead=0, in_pad=0, out_lead=0, out_pad=0, out=True, rec=True, status=True, status_in=None):
    """One check_stream through guarded buffers; returns (bytes or None, record or None, status or None)."""
    nf = frames.shape[0]
    b_in = Buf(api, nf, h.frame_bytes, in_pad, lead, rows=frames)
    b_out = Buf(api, nf, h.payload_bytes, out_pad, out_lead)            # handed in or not: it stays poisoned when it is not
    b_rec = Buf(api, 1, 2 * nf, item=4) if rec else None
    b_st = Buf(api, 1, nf, item=4) if status else None
    b_si = Buf(api, 1, nf, item=4, rows=[np.asarray(status_in, np.int32)]) if status_in is not None else None
    held = [b for b in (b_in, b_out, b_rec, b_st, b_si) if b is not None]
    try:
        k = h.check_stream(b_in.ptr, nf, b_out.ptr if out else None, b_rec and b_rec.ptr, b_st and b_st.ptr, b_si and b_si.ptr,
                           in_stride=h.frame_bytes + in_pad, out_stride=h.payload_bytes + out_pad)
        api.sync()
        assert k == nf
        b_in.intact()
        if b_si:
            b_si.intact()
        if not out:
            b_out.untouched()
        return (b_out.written() if out else None, b_rec.written(np.uint32).reshape(nf, 2) if rec else None,
                b_st.written(np.int32).reshape(nf) if status else None)
    finally:
        for b in held:
            b.free()


def append(api, h, pay, lead=0, in_pad=0, out_lead=0, out_pad=0):
    nf = pay.shape[0]
    b_in = Buf(api, nf, h.payload_bytes, in_pad, lead, rows=pay)
    b_out = Buf(api, nf, h.frame_bytes, out_pad, out_lead)
    try:
        k = h.append_stream(b_in.ptr, nf, b_out.ptr, in_stride=h.payload_bytes + in_pad, out_stride=h.frame_bytes + out_pad)
        api.sync()
        assert k == nf
        b_in.intact()
        return b_out.written()
    finally:
        b_in.free()
        b_out.free()


def same(got, want):
    return all(g is None or (g.dtype == w.dtype and np.array_equal(g, w)) for g, w in zip(got, want))


def damaged(frames):
    """Every third frame with one bit wrong, in the payload or in the tail."""
    f = frames.copy()
    for b in range(1, f.shape[0], 3):
        f[b, (b * 7919) % f.shape[1]] ^= np.uint8(1 << (b % 8))
    return f


# The four layouts of a call size, and five sets of optional buffers: all outputs and an upstream table; none but d_out; the
# record alone; all outputs; the status alone.  Each length takes the four layouts with four of the five sets, and the sets
# turn by one from a length to the next, so over the lengths every layout meets every set.
LAYOUTS = [dict(lead=lead, in_pad=1 + lead, out_lead=(3 * lead + 1) % 4, out_pad=4 - lead) for lead in range(4)]
OPTIONS = [dict(upstream=True), dict(rec=False, status=False), dict(out=False, status=False), dict(), dict(out=False, rec=False)]


@pytest.mark.parametrize("n_frames", [1, 3, 257])
@pytest.mark.parametrize("key", sorted(HANDLES))
def test_check_and_append_equal_the_plan(api, key, n_frames):
    """Every payload length, four layouts each: input leads of 0 .. 3 bytes, outputs at other byte offsets, strides 1 .. 4
    bytes beyond the row.  The two largest lengths run at three frames only."""
    model = HANDLES[key]
    for turn, P in enumerate(LENGTHS):
        if P in LARGEST and n_frames != 3:
            continue
        shape = (*model, P)
        pay = cc.rows(n_frames, P, P + n_frames)
        want_frames = api.crc_plan(*shape, data=pay)
        hit = damaged(want_frames)
        si = (np.arange(n_frames) % 5 == 2).astype(np.int32) * 9
        want, want_si = api.crc_plan(*shape, data=hit, verify=True), api.crc_plan(*shape, data=hit, verify=True, status_in=si)
        if model[0] and n_frames > 1:
            assert want[2][0] == 0 and want[2][1] == 1
        h = api.Crc(*shape)
        try:
            assert (h.payload_bytes, h.frame_bytes) == (P, P + model[0] // 8)
            for lay in LAYOUTS:
                opt = dict(OPTIONS[(lay["lead"] + turn) % len(OPTIONS)])
                up = opt.pop("upstream", False)
                got = check(api, h, hit, **lay, **opt, status_in=si if up else None)
                assert same(got, want_si if up else want), (key, P, n_frames, lay["lead"])
                assert np.array_equal(append(api, h, pay, **lay), want_frames), (key, P, n_frames, lay["lead"])
        finally:
            h.close()


def test_the_record_equals_zlib_and_crc_hqx(api):
    """Not via the plan: the computed CRC of the record against the two references every machine has."""
    for P, nf in ((1, 9), (5, 300), (1020, 64), (SHORT_MAX, 5), (SHORT_MAX + 1, 5), (65541, 3), (1 << 20, 2)):
        pay = cc.rows(nf, P, 3 * P)
        for model, ref in ((cc.model("CRC-32/ISO-HDLC"), lambda r: zlib.crc32(r.tobytes())),
                           (cc.model("CRC-16/XMODEM"), lambda r: binascii.crc_hqx(r.tobytes(), 0))):
            h = api.Crc(*model, *cc.PN_CCSDS, P)
            try:
                frames = append(api, h, pay, lead=1, in_pad=3, out_lead=2, out_pad=1)
                by, rec, st = check(api, h, frames, lead=3, in_pad=1, out_lead=1, out_pad=2)
                crcs = [ref(r) for r in pay]
                assert np.array_equal(by, pay) and not st.any() and rec[:, 0].tolist() == crcs and rec[:, 1].tolist() == crcs, (P, model)
            finally:
                h.close()


@pytest.mark.parametrize("case", ["65537 frames of 5 bytes", "more frames than a row of the grid"])
def test_more_frames_than_one_grid_row(api, case):
    """65 537 frames of 5 bytes; and 4 GRID_X + 5 frames of one byte, where the short class's groups no longer fit one row of
    the grid.  (A long-class call of more than GRID_X frames would take 4 GiB of rows and is not run: it shares the index
    expression.)"""
    nf, P, model = (65537, 5, cc.model("CRC-16/KERMIT")) if case.startswith("65537") else (4 * GRID_X + 5, 1, cc.model("CRC-8/SMBUS"))
    shape = (*model, *cc.PN_80211, P)
    pay = cc.rows(nf, P, nf)
    want_frames = api.crc_plan(*shape, data=pay)
    hit = want_frames.copy()
    hit[nf - 1, 0] ^= 1
    hit[GRID_X % nf, -1] ^= 2
    want = api.crc_plan(*shape, data=hit, verify=True)
    assert want[2].sum() == 2
    h = api.Crc(*shape)
    try:
        assert np.array_equal(append(api, h, pay, lead=1, in_pad=0, out_lead=3, out_pad=1), want_frames)
        assert same(check(api, h, hit, lead=3, in_pad=2, out_lead=1, out_pad=0), want)
    finally:
        h.close()


@pytest.mark.parametrize("P", [1021, SHORT_MAX + 3])
def test_runs_repeat_and_a_frame_depends_on_its_bytes_alone(api, P):
    """The same call twice; the same frames in another order, with another n_frames and other strides; every frame alone,
    as frame 0 of a one-frame call at another address parity."""
    shape = (*cc.model("CRC-32/ISCSI"), *cc.PN_LONG, P)
    nf = 11
    pay = cc.rows(nf, P, 21)
    h = api.Crc(*shape)
    try:
        fa = append(api, h, pay, lead=1, in_pad=2, out_lead=3, out_pad=1)
        assert np.array_equal(append(api, h, pay, lead=1, in_pad=2, out_lead=3, out_pad=1), fa) and np.array_equal(fa, api.crc_plan(*shape, data=pay))
        hit = damaged(fa)
        a = check(api, h, hit, lead=2, in_pad=3, out_lead=1, out_pad=2)
        assert same(check(api, h, hit, lead=2, in_pad=3, out_lead=1, out_pad=2), a) and same(a, api.crc_plan(*shape, data=hit, verify=True))
        order = np.random.default_rng(4).permutation(nf)[:7]
        assert same(check(api, h, hit[order], lead=3, in_pad=0, out_lead=0, out_pad=5), [v[order] for v in a])
        assert np.array_equal(append(api, h, pay[order], lead=0, in_pad=5, out_lead=1, out_pad=0), fa[order])
        for i in range(nf):
            one = check(api, h, hit[i:i + 1], lead=i % 4, in_pad=i % 3, out_lead=(i + 1) % 4, out_pad=i % 5)
            assert same(one, [v[i:i + 1] for v in a]), i
            assert np.array_equal(append(api, h, pay[i:i + 1], lead=(i + 2) % 4, in_pad=i % 5, out_lead=i % 4, out_pad=i % 3), fa[i:i + 1]), i
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
    """Nothing in a handle changes after create, so both calls are supported under graph capture: the two nodes -- a check
    and an append -- are replayed twice, the outputs poisoned again in between and an eager call on the same handle made
    between the replays, and both times the bytes equal the plan's."""
    hip = hip_runtime()
    P, nf = 1020, 9
    shape = (*cc.model("CRC-32/ISO-HDLC"), *cc.PN_CCSDS, P)
    pay = cc.rows(nf, P, 13)
    want_frames = api.crc_plan(*shape, data=pay)
    hit = damaged(want_frames)
    want = api.crc_plan(*shape, data=hit, verify=True)
    h = api.Crc(*shape)
    Fb = h.frame_bytes
    b_in, b_pay = Buf(api, nf, Fb, 3, 1, rows=hit), Buf(api, nf, P, 1, 3, rows=pay)
    b_out, b_rec, b_st, b_frm = Buf(api, nf, P, 2, 3), Buf(api, 1, 2 * nf, item=4), Buf(api, 1, nf, item=4), Buf(api, nf, Fb, 2, 1)
    s, g, ex = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert hip.hipStreamCreate(C.byref(s)) == 0
    assert hip.hipStreamBeginCapture(s, 0) == 0
    try:
        k = h.check_stream(b_in.ptr, nf, b_out.ptr, b_rec.ptr, b_st.ptr, in_stride=Fb + 3, out_stride=P + 2, stream=s.value)
        ka = h.append_stream(b_pay.ptr, nf, b_frm.ptr, in_stride=P + 1, out_stride=Fb + 2, stream=s.value)
    finally:
        ended = hip.hipStreamEndCapture(s, C.byref(g))
    assert ended == 0 and k == nf and ka == nf and hip.hipGraphInstantiate(C.byref(ex), g, None, None, 0) == 0
    try:
        for _ in range(2):
            for b in (b_out, b_rec, b_st, b_frm):
                b.poison()
            assert hip.hipGraphLaunch(ex, s) == 0 and hip.hipStreamSynchronize(s) == 0
            assert same((b_out.written(), b_rec.written(np.uint32).reshape(nf, 2), b_st.written(np.int32).reshape(nf)), want)
            assert np.array_equal(b_frm.written(), want_frames)
            b_in.intact()
            b_pay.intact()
            assert same(check(api, h, hit[:4], lead=1, in_pad=1), [v[:4] for v in want])          # an eager call between the replays
    finally:
        hip.hipGraphExecDestroy(ex)
        hip.hipGraphDestroy(g)
        hip.hipStreamDestroy(s)
        h.close()
        for b in (b_in, b_pay, b_out, b_rec, b_st, b_frm):
            b.free()


def test_refusals_launch_nothing(api, L):
    P, nf = 96, 3
    shape = (*cc.model("CRC-32/MPEG-2"), *cc.PN_CCSDS, P)
    frames = api.crc_plan(*shape, data=cc.rows(nf, P, 17))
    h = api.Crc(*shape)
    Fb = h.frame_bytes
    assert (h.payload_bytes, Fb) == (96, 100)
    d_in = api.DeviceArray.from_bytes(np.concatenate([frames.ravel(), np.zeros(64, np.uint8)]))
    poison = np.full(256, sc.POISON, np.uint32)
    d_out, d_rec, d_st, d_si = (sc._upload(api, poison) for _ in range(4))
    d_si.zero()
    lib = L.load()
    k = C.c_size_t(7)

    def call(pi=d_in.ptr, istride=Fb, psi=d_si.ptr, n=nf, po=d_out.ptr, ostride=P, pr=d_rec.ptr, ps=d_st.ptr, hh=None, kk=C.byref(k)):
        return lib.sfe_dsp_crc_check_stream(hh or h._h, pi, istride, psi, n, po, ostride, pr, ps, kk, None)

    def app(pi=d_in.ptr, istride=P, n=nf, po=d_out.ptr, ostride=Fb, hh=None, kk=C.byref(k)):
        return lib.sfe_dsp_crc_append_stream(hh or h._h, pi, istride, n, po, ostride, kk, None)

    def refused(rc, code, prefix):
        return rc == code and lib.sfe_dsp_last_error().startswith(prefix) and k.value == 0

    CHK, APP = b"crc_check_stream: ", b"crc_append_stream: "
    assert refused(call(istride=Fb - 1), L.SFE_ERANGE, CHK) and refused(call(ostride=P - 1), L.SFE_ERANGE, CHK)
    assert refused(app(istride=P - 1), L.SFE_ERANGE, APP) and refused(app(ostride=Fb - 1), L.SFE_ERANGE, APP)
    assert refused(call(pi=None), L.SFE_EINVAL, CHK) and refused(app(pi=None), L.SFE_EINVAL, APP) and refused(app(po=None), L.SFE_EINVAL, APP)
    assert refused(call(po=None, pr=None, ps=None), L.SFE_EINVAL, CHK)               # a call with no output
    assert refused(call(psi=d_si.ptr + 1), L.SFE_EINVAL, CHK)                        # misaligned, each of the four-byte buffers
    assert refused(call(pr=d_rec.ptr + 2), L.SFE_EINVAL, CHK) and refused(call(ps=d_st.ptr + 3), L.SFE_EINVAL, CHK)
    assert refused(call(n=1 << 31), L.SFE_EINVAL, CHK) and refused(app(n=1 << 31), L.SFE_EINVAL, APP)
    assert refused(call(istride=1 << 62), L.SFE_EINVAL, CHK) and refused(call(ostride=1 << 62), L.SFE_EINVAL, CHK)       # byte ranges that reach 2^62
    assert refused(app(istride=1 << 62), L.SFE_EINVAL, APP) and refused(app(ostride=1 << 62), L.SFE_EINVAL, APP)
    assert refused(call(po=d_in.ptr + nf * Fb - 1), L.SFE_EINVAL, CHK)               # each output over the input and over the status table
    assert refused(call(pr=d_in.ptr), L.SFE_EINVAL, CHK) and refused(call(ps=d_in.ptr + 8), L.SFE_EINVAL, CHK)
    assert refused(call(po=d_si.ptr + 4 * nf - 1), L.SFE_EINVAL, CHK) and refused(call(pr=d_si.ptr + 4), L.SFE_EINVAL, CHK)
    assert refused(call(ps=d_si.ptr), L.SFE_EINVAL, CHK)
    assert refused(call(pr=d_out.ptr + 8), L.SFE_EINVAL, CHK)                        # two outputs over one another
    assert refused(call(ps=d_out.ptr + 4 * ((nf * P - 1) // 4)), L.SFE_EINVAL, CHK) and refused(call(ps=d_rec.ptr + 4), L.SFE_EINVAL, CHK)
    assert refused(app(po=d_in.ptr + nf * P - 1), L.SFE_EINVAL, APP) and refused(app(pi=d_out.ptr + nf * Fb - 1), L.SFE_EINVAL, APP)
    assert call(kk=None) == L.SFE_EINVAL and lib.sfe_dsp_last_error().startswith(CHK)
    assert app(kk=None) == L.SFE_EINVAL and lib.sfe_dsp_last_error().startswith(APP)
    assert k.value == 0
    assert call(n=0) == L.SFE_OK and k.value == 0 and app(n=0) == L.SFE_OK and k.value == 0      # no frames: a no-op
    # a live handle of another block is refused, and crc's destroy frees nothing of it
    other = api.Corr(np.ones(13, np.complex64), 3840)
    assert refused(call(hh=other._h), L.SFE_EINVAL, CHK) and refused(app(hh=other._h), L.SFE_EINVAL, APP)
    assert lib.sfe_dsp_crc_destroy(other._h) == L.SFE_OK
    other.reset()                                                    # still alive
    other.close()
    with pytest.raises(AttributeError):
        h.reset()
    api.sync()
    for d in (d_out, d_rec, d_st):
        assert np.array_equal(sc._download(d), poison)
    # the next good call is a fresh handle's; the optional buffers may be left out
    want = api.crc_plan(*shape, data=frames, verify=True)
    assert call() == L.SFE_OK and k.value == nf
    assert call(psi=None, pr=None, ps=None) == L.SFE_OK and k.value == nf
    assert call(psi=None, po=None, pr=None) == L.SFE_OK and k.value == nf            # verify-only: the status alone
    api.sync()
    assert np.array_equal(d_out.to_numpy().view(np.uint8)[:nf * P].reshape(nf, P), want[0])
    assert np.array_equal(d_rec.to_numpy(2 * nf).view(np.uint32).reshape(nf, 2), want[1])
    assert np.array_equal(d_st.to_numpy(nf).view(np.int32), want[2])
    assert same(h.check(frames), want)
    assert np.array_equal(h.append(want[0]), frames)
    h.close()
    for d in (d_in, d_out, d_rec, d_st, d_si):
        d.free()


def test_the_chain_catches_a_miscorrection_on_the_device(api, L):
    """Crc.append -> Reed.encode_stream -> (channel) -> Reed.process_stream -> Crc.check on RS(7, 5), t = 1: only pointers and
    strides pass between the blocks.  Frame 0 is clean; frame 1 has one wrong byte, which reed repairs; frame 2 is a
    constructed miscorrection -- two of the three bytes in which its codeword differs from the codeword of a payload with
    one byte changed are overwritten with the other's, so the word lies at distance 1 from the WRONG codeword and reed
    returns it with status 0; a one-byte change is a burst of at most 8 bits, which a CRC-16 always catches.  Frame 3 has
    three wrong bytes: whatever reed says of it is handed on as d_status_in.  The scene is asserted on the CPU first,
    through the two host plans."""
    code = (0x11d, 0, 1, 7, 2, 1)
    P, nf = 3, 4
    shape = (*cc.model("CRC-16/XMODEM"), *cc.PN_CCSDS, P)
    pay = cc.rows(nf, P, 99)
    f5 = api.crc_plan(*shape, data=pay)                                 # reed's payloads
    sent = api.reed_plan(*code, data=f5, encode=True)
    other5 = f5[2].copy()
    other5[1] ^= 0x5A                                                   # the payload reed will believe in
    other = api.reed_plan(*code, data=other5, encode=True)[0]
    differ = np.flatnonzero(other != sent[2])
    assert differ.size == 3
    rx = sent.copy()
    rx[1, 4] ^= 0x21
    rx[2, differ[:2]] = other[differ[:2]]
    rx[3, [0, 3, 6]] ^= np.array([1, 2, 4], np.uint8)
    cpu5, cpu_rrec, cpu_rst = api.reed_plan(*code, data=rx)
    assert cpu_rst[:3].tolist() == [0, 0, 0] and np.array_equal(cpu5[:2], f5[:2]) and np.array_equal(cpu5[2], other5) and cpu_rrec[:3, 0].tolist() == [0, 1, 1]
    cpu = api.crc_plan(*shape, data=cpu5, verify=True, status_in=cpu_rst)
    assert cpu[2][:3].tolist() == [0, 0, 1] and cpu[2][3] == (2 if cpu_rst[3] else cpu[2][3]) and np.array_equal(cpu[0][:2], pay[:2])
    hc, hr = api.Crc(*shape), api.Reed(*code)
    assert (hc.frame_bytes, hr.payload_bytes, hr.frame_bytes) == (5, 5, 7)
    d_pay, d_f5, d_cw = api.DeviceArray.from_bytes(pay), api.DeviceArray(nf * 5 // 4 + 4), api.DeviceArray(nf * 7 // 4 + 4)
    d_r5, d_rrec, d_rst = api.DeviceArray(nf * 5 // 4 + 4), api.DeviceArray(2 * nf), api.DeviceArray(nf)
    d_out, d_rec, d_st = api.DeviceArray(nf * P // 4 + 4), api.DeviceArray(2 * nf), api.DeviceArray(nf)
    held = [d_pay, d_f5, d_cw, d_r5, d_rrec, d_rst, d_out, d_rec, d_st]
    try:
        assert hc.append_stream(d_pay, nf, d_f5) == nf
        assert hr.encode_stream(d_f5, nf, d_cw) == nf
        api.sync()
        on_air = d_cw.to_numpy().view(np.uint8)[:nf * 7].reshape(nf, 7).copy()
        assert np.array_equal(on_air, sent)
        api.check(d_cw._L.sfe_dsp_memcpy_h2d(d_cw.ptr, rx.ctypes.data, rx.nbytes, None))          # the channel
        api.sync()
        assert hr.process_stream(d_cw, nf, d_r5, d_rrec, d_rst) == nf
        assert hc.check_stream(d_r5, nf, d_out, d_rec, d_st, d_rst) == nf
        api.sync()
        r5 = d_r5.to_numpy().view(np.uint8)[:nf * 5].reshape(nf, 5)
        rst = d_rst.to_numpy().view(np.int32)
        out = d_out.to_numpy().view(np.uint8)[:nf * P].reshape(nf, P)
        rec, st = d_rec.to_numpy().view(np.uint32).reshape(nf, 2), d_st.to_numpy().view(np.int32)
    finally:
        for d in held:
            d.free()
        hc.close()
        hr.close()
    print("reed statuses", rst, "crc records", rec.tolist(), "crc statuses", st)
    assert np.array_equal(r5, cpu5) and np.array_equal(rst, cpu_rst)
    assert st[:3].tolist() == [0, 0, 1] and np.array_equal(out[:2], pay[:2]) and (out[2] != pay[2]).sum() == 1     # as received: one byte off
    assert same((out, rec, st), cpu)
