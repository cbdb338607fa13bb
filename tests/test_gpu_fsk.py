"""The 2-(G)FSK burst modem (sfe_dsp_fsk_*) on the GPU.  The bar is equality with api.fsk_plan -- float32 words, wire-format
bytes, packed bits, records and statuses -- never a tolerance.  The modulator's output sits between guards and is poisoned
before every call (tests/test_gpu_mod.py's Out); the demodulator's buffers are tests/stream_checks.py's guarded ones, every
output poisoned: after a call exactly the named slots are written.  The shapes of tests/fsk_cases.py, both output formats,
both input formats, every optional buffer given and NULL, overlapping windows, several streams, the statuses, the contracts
about bits, more timing candidates than the trees hold at once, the refusals, captured calls, and the loopback Fsk.mod ->
Corr -> Fsk.demod (-> Vit) on the device."""
import ctypes as C

import numpy as np
import pytest

import fsk_cases as fc
import mod_checks as mc
import stream_checks as sc
from simplefe_amd import synth
from test_gpu_mod import Out, hip_runtime, same
from test_gpu_mod import run as run_mod

pytestmark = pytest.mark.gpu
F32 = np.float32
POISON = np.uint32(sc.POISON)


@pytest.fixture(scope="module")
def api():
    from simplefe_amd import api as a
    return a


@pytest.fixture(scope="module")
def L():
    from simplefe_amd import lib
    return lib


@pytest.fixture(autouse=True)
def guards():
    yield
    sc.check_guarded()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def make(api, kw, **more):
    return api.Fsk(kw["sps"], kw["pulse"], kw["h"], kw["pre"], kw["n_bits"], kw["mf"], kw["delay"], kw["rng"], kw["amp"], kw["scale"],
                   kw["min_gate"], kw["out_fmt"], **more)


def slots(raw_u8, n_rows, row_bytes, stride_bytes, what):
    """The rows of a read-back output (uint8) laid at stride_bytes, after checking that every byte outside them kept the poison."""
    poison = np.full((raw_u8.size + 3) // 4, POISON, np.uint32).view(np.uint8)[:raw_u8.size]
    inside = np.zeros(raw_u8.size, bool)
    rows = np.empty((n_rows, row_bytes), np.uint8)
    for r in range(n_rows):
        inside[r * stride_bytes:r * stride_bytes + row_bytes] = True
        rows[r] = raw_u8[r * stride_bytes:r * stride_bytes + row_bytes]
    assert (raw_u8[~inside] == poison[~inside]).all(), "a store outside the %s slots" % what
    return rows


def run_demod(api, h, x, nb, idx=None, gate=None, base=0, step=0, pad=0, bits=True, rec=True, status=True, stream=None, held=None):
    """One demod call on guarded buffers: x is (S, n) complex64, or (S, 2n) uint8 on a handle set to FMT_U8.  Strides are the
    rows + pad.  Returns (soft (S, nb, n_bits), bytes or None, record or None, status or None) after checking the poison."""
    S, nbit, nby = h.n_streams, h.n_bits, h.n_bytes
    x = np.ascontiguousarray(x).reshape(S, -1)
    n = x.shape[1] // 2 if h.in_u8 else x.shape[1]
    istride, sstride, bstride, ststride = n + pad, nbit + pad, nby + pad, nb + pad
    if h.in_u8:
        buf = np.full((S, 2 * istride), 0x80, np.uint8)
        buf[:, :2 * n] = x
        d_in = sc.from_bytes(api, buf)
    else:
        buf = np.full((S, istride), np.complex64(9 - 9j), np.complex64)
        buf[:, :n] = x
        d_in = sc.from_numpy(api, buf.view(F32))
    d_idx = d_gate = None
    if idx is not None:
        lay = np.full((S, ststride), 0xFFFFFFFF, np.uint32)
        lay[:, :nb] = np.asarray(idx, np.uint32).reshape(S, nb)
        d_idx = sc.from_numpy(api, lay.view(F32))
    if gate is not None:
        lay = np.full((S, ststride), np.nan, F32)
        lay[:, :nb] = np.asarray(gate, F32).reshape(S, nb)
        d_gate = sc.from_numpy(api, lay)
    rows = S * nb
    d_soft = sc.device_array(api, rows * sstride)
    d_by = sc.device_array(api, (rows * bstride + 3) // 4) if bits else None
    d_rec = sc.device_array(api, rows * 8) if rec else None
    d_st = sc.device_array(api, S * ststride) if status else None
    call = lambda: h.demod(d_in, n, nb, d_soft, d_by, d_idx, d_gate, d_rec, d_st, base, step, in_stride=istride, idx_stride=ststride,
                           gate_stride=ststride, soft_stride=sstride, bits_stride=bstride, status_stride=ststride, stream=stream)
    if held is not None:            # the caller runs the call itself (a capture)
        held.extend([d_soft, d_by, d_rec, d_st])
        return call
    assert call() == nb
    api.sync()
    return read_demod(h, nb, pad, d_soft, d_by, d_rec, d_st)


def read_demod(h, nb, pad, d_soft, d_by, d_rec, d_st):
    S, nbit, nby = h.n_streams, h.n_bits, h.n_bytes
    rows = S * nb
    soft = slots(d_soft.to_numpy(keep=True).view(np.uint8), rows, 4 * nbit, 4 * (nbit + pad), "soft").view(F32).reshape(S, nb, nbit)
    assert not (_bits(soft) == POISON).any(), "soft values never stored"
    by = rec = st = None
    if d_by is not None:
        raw = d_by.to_numpy(keep=True).view(np.uint8)
        by = slots(raw[:rows * (nby + pad)], rows, nby, nby + pad, "bits").reshape(S, nb, nby)
        assert (raw[rows * (nby + pad):] == np.full(raw.size // 4, POISON, np.uint32).view(np.uint8)[rows * (nby + pad):]).all()
    if d_rec is not None:
        rec = d_rec.to_numpy(keep=True).reshape(S, nb, 8)
        assert not (_bits(rec) == POISON).any()
    if d_st is not None:
        st = slots(d_st.to_numpy(keep=True).view(np.uint8), S, 4 * nb, 4 * (nb + pad), "status").view(np.int32).reshape(S, nb)
        assert not (st.view(np.uint32) == POISON).any()
    return soft, by, rec, st


def plan_demod(api, kw, x, nb, idx=None, gate=None, base=0, step=0):
    """The plan on every stream of x (S, n) complex64: the same four arrays as run_demod."""
    x = np.atleast_2d(x)
    outs = [api.fsk_plan(**kw, x=x[s], idx=None if idx is None else np.reshape(idx, (x.shape[0], nb))[s],
                         gate=None if gate is None else np.reshape(gate, (x.shape[0], nb))[s], n_bursts=nb, start_base=base, start_step=step)
            for s in range(x.shape[0])]
    return tuple(np.stack([o[i] for o in outs]) for i in range(4))


def equal(got, want):
    for g, w, name in zip(got, want, ("soft", "bits", "record", "status")):
        if g is None:
            continue
        assert g.shape == w.shape and np.array_equal(g.view(np.uint8), w.view(np.uint8)), "%s differs from the plan's" % name


def received(api, kw, nb, seed, at=37, gap=23, snr_db=20.0, f=0.004, streams=1):
    """nb frames of the plan's waveform `gap` samples apart from sample `at` on, a carrier offset, noise: (x (streams, n)
    complex64, the payloads (streams, nb, n_bytes), the step between frames)."""
    N, F, _, _ = api.fsk_plan(**kw)
    step = F + gap
    n = at + nb * step + 64
    xs, ds = [], []
    for s in range(streams):
        data = fc.payload_clean(kw["n_bits"], nb, seed + 17 * s)
        y = api.fsk_plan(**kw, data=data, n_out=n, start_base=at, start_step=step)
        xs.append(fc.channel(y, n, 0, f=f, phase=0.3 + s, snr_db=snr_db, seed=seed + s, amp=kw["amp"]).astype(np.complex64))
        ds.append(data)
    return np.stack(xs), np.stack(ds), step


# ------------------------------------------------------------------------------------------------ the modulator
@pytest.mark.parametrize("s", fc.GPU_SHAPES, ids=fc.GPU_IDS)
def test_mod_equals_the_plan(api, L, s):
    """Every shape, F32 at both 16-byte phases of its address and TX10 with frames that start mid-group (an odd start_base, an
    odd step): frames that touch, frames with gaps, a tail; the payload rows at a stride of their own."""
    nb = s[5]
    for fmt, shift in ((L.FMT_F32, 8), (L.FMT_F32, 0), (L.FMT_TX10, 3)):
        kw = fc.gpu_shape(s, out_fmt=fmt, amp=0.75)
        h = make(api, kw)
        F = h.frame_len
        data = fc.payload(kw["n_bits"], nb, F)
        for base, step, tail in ((0, F, 0), (5, F + 3, 12), (1029, F + 2000, 1)):
            n_out = base + (nb - 1) * step + F + tail
            place = dict(n_out=n_out + n_out % 2, start_base=base, start_step=step)
            want = api.fsk_plan(**kw, data=data, **place)
            got = run_mod(api, h, data, in_pad=3, lead=1, shift=shift, call=h.mod, **place)
            assert same(got, want), (s[:3], fmt, base, step)
        h.close()


def test_no_bursts_write_zeros(api, L):
    for fmt in (L.FMT_F32, L.FMT_TX10):
        kw = fc.gpu_shape(fc.GPU_SHAPES[1], out_fmt=fmt)
        h = make(api, kw)
        out = Out(api, 3000, fmt == L.FMT_TX10, 0)
        assert h.mod(None, 0, out.ptr, 3000) == 3000
        api.sync()
        got = out.take()
        assert same(got, api.fsk_plan(**kw, data=np.zeros((0, 8), np.uint8), n_out=3000))
        assert not synth.tx10_unpack(got).any() if fmt == L.FMT_TX10 else not got.view(np.uint32).any()
        out.free()
        h.close()


def test_a_frame_depends_on_its_bytes_alone(api, L):
    """The same bytes at another b, another stride and another offset of the stream give the same words; a second run repeats."""
    kw = fc.gpu_shape(fc.GPU_SHAPES[2])
    h = make(api, kw)
    F, nby = h.frame_len, h.n_bytes
    data = fc.payload(kw["n_bits"], 4, 5)
    a = run_mod(api, h, data, 4 * (F + 6) + 10, 3, F + 6, call=h.mod)
    again = run_mod(api, h, data, 4 * (F + 6) + 10, 3, F + 6, call=h.mod)
    assert same(a, again)
    moved = run_mod(api, h, data[[2, 0, 3, 1]], 1030 + 4 * (F + 1000), 1030, F + 1000, in_pad=5, lead=3, shift=8, call=h.mod)
    for b, src in enumerate([2, 0, 3, 1]):
        assert same(moved[1030 + b * (F + 1000):][:F], a[3 + src * (F + 6):][:F]), (b, src)
    assert nby == 13
    h.close()


# ------------------------------------------------------------------------------------------------ the demodulator
@pytest.mark.parametrize("s", fc.GPU_SHAPES, ids=fc.GPU_IDS)
def test_demod_equals_the_plan(api, L, s):
    """Every shape on the plan's waveform plus seeded noise, R in {0, 2, sps}, indices and gates given, strides beyond the rows;
    cf32, and u8 -- whose outputs equal the cf32 path's on the converted samples, i.e. the plan's on them."""
    sps, nb = s[0], s[5]
    for R in (0, 2, sps):
        kw = fc.gpu_shape(s, rng=R, scale=4.0, min_gate=0.5)
        x, data, step = received(api, kw, nb, seed=R + sps, at=40 + R)
        idx = np.arange(nb, dtype=np.uint32) % 3                # the windows start 0, 1 or 2 samples late: inside R or not
        gate = np.linspace(0.6, 2.0, nb).astype(F32)
        h = make(api, kw)
        got = run_demod(api, h, x, nb, idx, gate, base=40 + R, step=step, pad=3)
        want = plan_demod(api, kw, x, nb, idx, gate, base=40 + R, step=step)
        equal(got, want)
        assert not want[3].any()
        if R == sps:                                            # timing has the room: the bytes come back
            assert np.array_equal(got[1][0], data[0]), (s[:3], R)
        if R == 2:
            b8, x8 = fc.f32_as_u8_samples(0.5 * x)
            h.set_input_format(L.FMT_U8)
            got8 = run_demod(api, h, b8.reshape(1, -1), nb, idx, gate, base=40 + R, step=step, pad=1)
            equal(got8, plan_demod(api, kw, x8.reshape(1, -1), nb, idx, gate, base=40 + R, step=step))
        h.close()


def test_more_candidates_than_the_trees_hold_at_once(api, L):
    """Lp = 100 pads to 128 words, so 32 candidates fit the trees; R = 20 asks for 41: two passes, the best in either."""
    pre = np.random.default_rng(3).integers(0, 2, 100).tolist()
    kw = fc.shape(4, 0.5, 3, pre=pre, n_bits=40, rng=20)
    h = make(api, kw)
    for late in (0, 19, 37):                                    # the best candidate in the first pass, and in the second
        x, data, step = received(api, kw, 2, seed=late, at=60)
        got = run_demod(api, h, x, 2, base=60 - 18 + late, step=step)
        want = plan_demod(api, kw, x, 2, base=60 - 18 + late, step=step)
        equal(got, want)
        assert want[2][0, 0, 0] == 18 - late and np.array_equal(got[1][0], data[0])
    h.close()


def test_every_optional_buffer_given_and_null(api, L):
    kw = fc.gpu_shape(fc.GPU_SHAPES[1])
    x, data, step = received(api, kw, 3, seed=2)
    h = make(api, kw)
    idx, gate = np.array([0, 1, 0], np.uint32), np.ones(3, F32)
    want = plan_demod(api, kw, x, 3, idx, gate, 37, step)
    for drop in ("idx", "gate", "bits", "rec", "status", None):
        got = run_demod(api, h, x, 3, None if drop == "idx" else idx, None if drop == "gate" else gate, 37, step, bits=drop != "bits",
                        rec=drop != "rec", status=drop != "status")
        equal(got, plan_demod(api, kw, x, 3, None, gate, 37, step) if drop == "idx" else want)
    h.close()


def test_overlapping_windows_and_streams_with_strides(api, L):
    """Windows one sample apart read the same samples; three streams at a stride beyond n_in; a burst's outputs do not depend
    on b, s or n_bursts: the same reach elsewhere gives the same words."""
    kw = fc.gpu_shape(fc.GPU_SHAPES[1], rng=2)
    x, data, step = received(api, kw, 2, seed=4, streams=3)
    h1, h3 = make(api, kw), make(api, kw, n_streams=3)
    got = run_demod(api, h3, x, 5, base=35, step=1, pad=7)       # windows at 35 .. 39: the frame at 37 is inside R of each
    want = plan_demod(api, kw, x, 5, base=35, step=1)
    equal(got, want)
    print("tau of the five overlapping windows, per stream:", got[2][:, :, 0].tolist())
    # stream 1's second frame as stream 0's only burst, at another offset of another buffer
    moved = np.concatenate([np.zeros(5, np.complex64), x[1, 37 + step - 20:]])
    one = run_demod(api, h1, moved[None, :], 1, base=25)
    two = run_demod(api, h3, x, 2, base=37, step=step)
    for g, w in zip(one, two):
        assert np.array_equal(g[0, :1].view(np.uint8), w[1, 1:].view(np.uint8))
    h1.close()
    h3.close()


def test_statuses_in_one_call_leave_their_neighbours_alone(api, L):
    kw = fc.gpu_shape(fc.GPU_SHAPES[1], min_gate=0.5)
    nb = 6
    x, data, step = received(api, kw, nb, seed=6)
    x[0, 37 + step + 100] = np.nan                               # burst 1: a NaN in its reach
    x[0, 37 + 4 * step + 90] = np.complex64(complex(0, np.inf))  # burst 4
    gate = np.array([1, 1, 0.25, np.nan, 1, 1], F32)             # bursts 2 and 3 are gated
    idx = np.array([0, 0, 0, 0, 0, 1 << 20], np.uint32)          # burst 5 leaves the stream behind
    h = make(api, kw)
    got = run_demod(api, h, x, nb, idx, gate, 37, step)
    equal(got, plan_demod(api, kw, x, nb, idx, gate, 37, step))
    assert got[3][0].tolist() == [0, 1, 2, 2, 1, 3]
    assert np.array_equal(got[1][0, 0], data[0, 0])
    for b in range(1, nb):
        assert not got[0][0, b].view(np.uint32).any() and not got[1][0, b].any()
        assert np.isnan(got[2][0, b, :4]).all() and not got[2][0, b, 4:].view(np.uint32).any()
    front = run_demod(api, h, x, 2, None, None, 37 - step, step)        # burst 0 starts before the stream
    equal(front, plan_demod(api, kw, x, 2, None, None, 37 - step, step))
    assert front[3][0].tolist() == [3, 0]
    h.close()


def test_refusals_launch_nothing(api, L):
    kw = fc.gpu_shape(fc.GPU_SHAPES[1])
    h, ht = make(api, kw), make(api, dict(kw, out_fmt=L.FMT_TX10))
    F, nby, nbit, nb = h.frame_len, h.n_bytes, h.n_bits, 3
    lib = L.load()
    k = C.c_size_t(7)
    x, data, step = received(api, kw, nb, seed=1)
    n, data = x.shape[1], data[0]
    d_x, d_data = sc.from_numpy(api, x.view(F32)), sc.from_bytes(api, np.concatenate([data.ravel(), np.zeros(64, np.uint8)]))
    d_soft, d_by, d_rec, d_st = sc.device_array(api, nb * nbit), sc.device_array(api, nb * nby), sc.device_array(api, nb * 8), sc.device_array(api, nb)
    n_out = nb * F + 7                                           # even: F is odd
    out = Out(api, n_out, False, 0)

    def mod(pi=d_data.ptr, istride=nby, n_bursts=nb, base=2, step_=F, po=out.ptr, n_=n_out, hh=h._h, kk=C.byref(k)):
        return lib.sfe_dsp_fsk_mod_stream(hh, pi, istride, n_bursts, base, step_, po, n_, kk, None)

    assert mod(istride=nby - 1) == L.SFE_ERANGE and lib.sfe_dsp_last_error().startswith(b"fsk_mod_stream: ")
    for rc in (mod(pi=None), mod(po=None), mod(po=out.ptr + 4), mod(base=-1), mod(step_=F - 1), mod(base=9), mod(n_=n_out - 6), mod(n_=1 << 31),
               mod(n_bursts=1 << 31), mod(hh=ht._h, n_=n_out - 1), mod(n_bursts=2, istride=1 << 62), mod(po=d_data.ptr), mod(pi=out.ptr + 8 * n_out - 1),
               mod(kk=None), mod(hh=None)):
        assert rc == L.SFE_EINVAL
    assert k.value == 0

    def dem(pi=d_x.ptr, n_in=n, istride=n, px=None, pg=None, n_bursts=nb, base=37, po=d_soft.ptr, sstride=nbit, pb=d_by.ptr, bstride=nby,
            pr=d_rec.ptr, ps=d_st.ptr, ststride=nb, hh=h._h, kk=C.byref(k)):
        return lib.sfe_dsp_fsk_demod_stream(hh, pi, n_in, istride, px, nb, pg, nb, n_bursts, base, step, po, sstride, pb, bstride, pr, ps, ststride, kk,
                                            None)

    for rc in (dem(sstride=nbit - 1), dem(bstride=nby - 1), dem(ststride=nb - 1)):
        assert rc == L.SFE_ERANGE and lib.sfe_dsp_last_error().startswith(b"fsk_demod_stream: ")
    for rc in (dem(pi=None), dem(po=None), dem(pi=d_x.ptr + 4), dem(po=d_soft.ptr + 2), dem(pr=d_rec.ptr + 1), dem(ps=d_st.ptr + 2),
               dem(px=d_x.ptr + 2), dem(n_in=1 << 31), dem(n_bursts=1 << 31), dem(base=(1 << 63) - 1), dem(sstride=1 << 61),
               dem(po=d_x.ptr), dem(pb=d_x.ptr + 1), dem(pr=d_soft.ptr), dem(ps=d_by.ptr), dem(px=d_st.ptr), dem(pg=d_rec.ptr), dem(pb=d_soft.ptr + 5),
               dem(kk=None), dem(hh=None)):
        assert rc == L.SFE_EINVAL
    assert k.value == 0
    other = api.Corr(np.ones(13, np.complex64), 3840)
    assert dem(hh=other._h) == L.SFE_EINVAL and mod(hh=other._h) == L.SFE_EINVAL
    other.close()
    with pytest.raises(AttributeError):
        h.reset()
    with pytest.raises(L.SfeError):
        h.set_input_format(L.FMT_TX10)
    api.sync()
    assert (out.d.to_numpy().view(np.uint32) == sc.POISON).all()
    for d in (d_soft, d_by, d_rec, d_st):
        assert (d.to_numpy(keep=True).view(np.uint32) == sc.POISON).all()
    # the next good calls are a fresh handle's
    assert mod() == L.SFE_OK and k.value == n_out and dem() == L.SFE_OK and k.value == nb
    api.sync()
    assert same(out.take(), api.fsk_plan(**kw, data=data, n_out=n_out, start_base=2, start_step=F))
    equal(read_demod(h, nb, 0, d_soft, d_by, d_rec, d_st), plan_demod(api, kw, x, nb, base=37, step=step))
    assert dem(n_bursts=0, pi=None, po=None) == L.SFE_OK and k.value == 0
    # the host conveniences
    assert same(h.modulate(data, n_out, 2, F), api.fsk_plan(**kw, data=data, n_out=n_out, start_base=2, start_step=F))
    equal(h.demodulate(x, n_bursts=nb, start_base=37, start_step=step), plan_demod(api, kw, x, nb, base=37, step=step))
    out.free()
    h.close()
    ht.close()


def test_captured_calls_replay_onto_poisoned_outputs(api, L):
    """Everything a call uses travels by value and the handle's tables never change: both calls may be captured.  Each node is
    replayed twice onto poisoned outputs and reproduces the eager bits, the plan's."""
    hip = hip_runtime()
    kw = fc.gpu_shape(fc.GPU_SHAPES[2])
    nb = 3
    x, data, step = received(api, kw, nb, seed=8)
    h = make(api, kw)
    F = h.frame_len
    place = dict(n_out=nb * (F + 7) + 40, start_base=11, start_step=F + 7)
    want_mod = api.fsk_plan(**kw, data=data[0], **place)
    want_dem = plan_demod(api, kw, x, nb, base=37, step=step)
    d_in, out = api.DeviceArray.from_bytes(data[0]), Out(api, place["n_out"], False, 8)
    outs = []
    s, g, ex = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert hip.hipStreamCreate(C.byref(s)) == 0
    call = run_demod(api, h, x, nb, base=37, step=step, stream=s.value, held=outs)
    assert hip.hipStreamBeginCapture(s, 0) == 0
    try:
        k1 = h.mod(d_in, nb, out.ptr, place["n_out"], place["start_base"], place["start_step"], stream=s.value)
        k2 = call()
    finally:
        ended = hip.hipStreamEndCapture(s, C.byref(g))
    assert ended == 0 and k1 == place["n_out"] and k2 == nb and hip.hipGraphInstantiate(C.byref(ex), g, None, None, 0) == 0
    try:
        for _ in range(2):
            out.poison()
            for d in outs:
                d.to_numpy()                                    # reading an output poisons it again
            assert hip.hipGraphLaunch(ex, s) == 0 and hip.hipStreamSynchronize(s) == 0
            assert same(out.take(), want_mod)
            equal(read_demod(h, nb, 0, *outs), want_dem)
    finally:
        hip.hipGraphExecDestroy(ex)
        hip.hipGraphDestroy(g)
        hip.hipStreamDestroy(s)
        h.close()
        d_in.free()
        out.free()


# ------------------------------------------------------------------------------------------------ the loopback
@pytest.mark.parametrize("fmt", ["f32", "tx10-as-u8"])
def test_loopback_returns_the_bytes_that_went_in(api, L, fmt):
    """Vit's encoder (host) -> Fsk.mod -> Corr -> Fsk.demod -> Vit (SOFT) on the device: one template, the plan's modulated
    preamble; d_peak_idx and d_peak_val as they lie are d_idx and d_gate.  The packed bits are the coded bytes that went in,
    and the decoder behind the soft values returns the payload.  With TX10 the receive side reads a host-side requantisation
    of the wire format to (I,Q) bytes: there is no TX10 -> u8 converter on the device."""
    K, gen, n_info, nb, block, base = 7, (0o171, 0o133), 106, 4, 3840, 100
    u8 = fmt != "f32"
    kw = fc.shape(10, 0.3, 4, pre=fc.PRE24, n_bits=2 * (n_info + K - 1), amp=0.5, scale=2.0, min_gate=0.5,
                  out_fmt=L.FMT_TX10 if u8 else L.FMT_F32)
    pay = [synth.vit_bits(n_info, 30 + b) for b in range(nb)]
    coded = np.stack([np.packbits(np.asarray(api.vit_encode(K, gen, bits), np.uint8)) for bits in pay])
    hm = make(api, kw)
    F, tpl_len = hm.frame_len, (len(fc.PRE24) - 1) * 10
    tpl = api.fsk_plan(**dict(kw, out_fmt=L.FMT_F32), data=coded[:1], n_out=F)[:tpl_len]
    hc = api.Corr(tpl, block, min_energy=1e-3)
    hv = api.Vit(K, gen, n_info, in_mode=L.VIT_IN_SOFT)
    if u8:
        hc.set_input_format(L.FMT_U8)
        hm.set_input_format(L.FMT_U8)
    n_out = nb * block
    d_data, out = api.DeviceArray.from_bytes(coded), Out(api, n_out, u8, 0)
    d_val, d_idx = api.DeviceArray(nb), api.DeviceArray(nb)
    d_soft, d_cb, d_frec, d_fst = api.DeviceArray(nb * hm.n_bits), api.DeviceArray(nb * hm.n_bytes // 4 + 1), api.DeviceArray(nb * 8), api.DeviceArray(nb)
    d_by, d_rec, d_st = api.DeviceArray((nb * hv.n_bytes + 3) // 4), api.DeviceArray(2 * nb), api.DeviceArray(nb)
    held = [d_data, out, d_val, d_idx, d_soft, d_cb, d_frec, d_fst, d_by, d_rec, d_st]
    try:
        assert hm.mod(d_data, nb, out.ptr, n_out, base, block) == n_out
        x = out.ptr
        if u8:
            api.sync()
            held.append(api.DeviceArray.from_bytes(mc.tx10_as_u8_samples(out.take())))
            x = held[-1].ptr
        assert hc.process_stream(x, n_out, d_val, d_idx) == nb
        assert hm.demod(x, n_out, nb, d_soft, d_cb, d_idx, d_val, d_frec, d_fst, start_base=-(tpl_len - 1), start_step=block) == nb
        assert hv.process_stream(d_soft, nb, d_by, d_rec, d_st, d_fst, in_stride=hm.n_bits) == nb
        api.sync()
        idx, val = d_idx.to_numpy().view(np.uint32), d_val.to_numpy()
        cb = d_cb.to_numpy().view(np.uint8)[:nb * hm.n_bytes].reshape(nb, hm.n_bytes)
        frec, fst = d_frec.to_numpy().reshape(nb, 8), d_fst.to_numpy().view(np.int32)
        by = d_by.to_numpy().view(np.uint8)[:nb * hv.n_bytes].reshape(nb, hv.n_bytes)
        st = d_st.to_numpy().view(np.int32)
    finally:
        for d in held:
            d.free()
        for h in (hm, hc, hv):
            h.close()
    print(fmt, "corr indices", idx, "values", val, "fsk statuses", fst, "tau", frec[:, 0], "dev", frec[:, 2], "vit statuses", st)
    assert idx.tolist() == [base + tpl_len - 1] * nb
    assert not fst.any() and not st.any()
    assert np.array_equal(cb, coded)
    assert np.array_equal(by, np.stack([synth.vit_pack(b) for b in pay]))
