"""The QAM mapper and soft demapper (sfe_dsp_qam_*) on the GPU.  The bar is equality with api.qam_plan -- float32 words --
never a tolerance.  Every buffer sits between guards (tests/stream_checks.py), every output is poisoned before the call:
after it exactly the floats (demap) or cf32 (map) of each row are written, the words between rows and the guards keep their
poison, and the inputs are what was uploaded.  Every order at every row length, strides exact and exact + 1 (which takes
every second row off its 16-byte boundary and the kernels down their fallback paths), perm none, reversal and random, csi
periods 0, 1, 52 of 64 and 4096; rows longer than a workgroup's tile; more workgroups than one grid row; the contracts about
bits; the refusals; a captured call; and the chain Ldpc.encode_stream -> Qam.map_stream -> OfdmMod (SYMBOLS) -> (the channel,
on the host: it is no block) -> Ofdm (ZF, d_chan) -> Qam.demap_stream -> Ldpc.process_stream with no host copy between the
blocks of either side."""
import ctypes as C

import numpy as np
import pytest

import ldpc_cases as lc
import ofdmmod_cases as mc
import qam_cases as qc
import stream_checks as sc

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


def lay(rows, stride, lead, fill):
    """rows (n, w) laid at `stride` elements behind `lead` elements, the rest `fill`."""
    n, w = rows.shape
    buf = np.full(lead + n * stride + 2, fill, rows.dtype)
    for r in range(n):
        buf[lead + r * stride:][:w] = rows[r]
    return buf


def taken(d_out, words_per_elem, n_rows, row_elems, stride, lead):
    """The rows of a guarded, poisoned output as uint32 (n_rows, row_elems * words_per_elem), after checking that every word
    outside them kept its poison.  (A computed word equal to the poison would be a NaN of one payload: none here.)"""
    raw = d_out.to_numpy(keep=True).view(np.uint32)
    w, k = words_per_elem, words_per_elem * row_elems
    inside = np.zeros(raw.size, bool)
    rows = np.empty((n_rows, k), np.uint32)
    for r in range(n_rows):
        a = w * (lead + r * stride)
        inside[a:a + k] = True
        rows[r] = raw[a:a + k]
    assert (raw[~inside] == POISON).all(), "a store outside the rows, the first at word %d" % int(np.flatnonzero((raw != POISON) & ~inside)[0])
    assert not (rows == POISON).any(), "%d words of the rows were never stored" % int((rows == POISON).sum())
    return rows


def run_demap(api, h, z, csi=None, pad=0, lead=0, csi_pad=0):
    """One demap call on guarded buffers: rows `lead` elements into their buffers at strides of the row + pad."""
    nr, ns = z.shape
    zs, os_ = ns + pad, h.n_bits + pad
    d_z = sc.from_numpy(api, lay(z, zs, lead, np.complex64(7 - 7j)).view(F32))
    d_h, cs = None, None
    if csi is not None:
        cs = csi.shape[1] + csi_pad
        d_h = sc.from_numpy(api, lay(csi, cs, lead, np.complex64(1e9)).view(F32))
    d_o = sc.device_array(api, lead + nr * os_ + 2)
    k = h.demap_stream(d_z.ptr + 8 * lead, nr, d_o.ptr + 4 * lead, None if d_h is None else d_h.ptr + 8 * lead, in_stride=zs, csi_stride=cs,
                       out_stride=os_)
    api.sync()
    assert k == nr
    rows = taken(d_o, 1, nr, h.n_bits, os_, lead)
    for d in (d_z, d_h, d_o):
        if d is not None:
            d.free()                # the guards and the inputs' contents are checked here
    return rows.view(F32)


def run_map(api, h, data, pad=0, lead=0):
    nr = data.shape[0]
    bs, os_ = h.n_bytes + pad, h.n_sym + pad
    d_b = sc.from_bytes(api, lay(data[:, :h.n_bytes], bs, lead, np.uint8(0x5A)))
    d_o = sc.device_array(api, 2 * (lead + nr * os_ + 2))
    k = h.map_stream(d_b.ptr + lead, nr, d_o.ptr + 8 * lead, in_stride=bs, out_stride=os_)
    api.sync()
    assert k == nr
    rows = taken(d_o, 2, nr, h.n_sym, os_, lead)
    d_b.free()
    d_o.free()
    return rows.view(np.complex64)


def both_directions(api, order, n_sym, n_rows, pad, pk, period, seed=0, amp=0.9, scale=1.5):
    B = n_sym * qc.BPS[order]
    perm = qc.perm_of(pk, B, seed)
    idx, clen, csi = qc.csi_of(period, n_rows, seed)
    h = api.Qam(order, n_sym, amp, scale, perm, idx, clen)
    try:
        z = qc.noisy_symbols(order, n_rows, n_sym, amp, 0.4, seed)
        want = api.qam_plan(order, n_sym, amp, scale, perm, idx, clen, sym=z, csi=csi)
        got = run_demap(api, h, z, csi, pad=pad, lead=pad, csi_pad=pad)
        assert np.array_equal(_bits(got), _bits(want)), ("demap", order, n_sym, n_rows, pad, pk, period)
        data = qc.coded_bytes(n_rows, h.n_bytes, seed)
        want = api.qam_plan(order, n_sym, amp, scale, perm, data=data)
        got = run_map(api, h, data, pad=pad, lead=3 * pad)
        assert np.array_equal(_bits(got), _bits(want)), ("map", order, n_sym, n_rows, pad, pk, period)
    finally:
        h.close()


# (n_rows, stride pad, perm, csi_period): every pair of values of any two of the four stands in some row
COMBOS = [(1, 0, "none", 0), (5, 1, "reversal", 1), (300, 0, "random", 52), (1, 1, "random", 4096), (5, 0, "none", 52), (300, 1, "reversal", 4096),
          (1, 0, "reversal", 52), (5, 1, "random", 0), (300, 0, "none", 1), (1, 1, "none", 4096), (5, 0, "random", 1), (300, 1, "none", 0),
          (1, 1, "reversal", 0), (5, 0, "reversal", 4096), (300, 1, "random", 1), (1, 0, "random", 1), (5, 1, "none", 52), (300, 0, "reversal", 0)]
N_SYMS = (1, 3, 63, 64, 65, 257, 1000)


def test_the_combinations_cover_every_pair():
    vals = [(1, 5, 300), (0, 1), ("none", "reversal", "random"), (0, 1, 52, 4096)]
    for i in range(4):
        for j in range(i + 1, 4):
            assert {(c[i], c[j]) for c in COMBOS} == {(a, b) for a in vals[i] for b in vals[j]}, (i, j)


@pytest.mark.parametrize("n_sym", N_SYMS)
@pytest.mark.parametrize("order", qc.ORDERS)
def test_device_equals_plan_both_directions(api, order, n_sym):
    """Every order at every row length; each takes six of the eighteen combinations of (rows, stride, perm, csi), in turn, so
    that every combination runs at some order and length many times over and every order meets every value of each."""
    at = 6 * (qc.ORDERS.index(order) + 5 * N_SYMS.index(n_sym))
    for j in range(6):
        n_rows, pad, pk, period = COMBOS[(at + j) % len(COMBOS)]
        both_directions(api, order, n_sym, n_rows, pad, pk, period, seed=j)


@pytest.mark.parametrize("order", qc.ORDERS)
def test_rows_longer_than_a_tile(api, order):
    """A workgroup takes 2048 symbols of a row: one symbol less, exactly, one more, and several tiles with a short last one;
    the residues q mod csi_period start anywhere in a later tile, and with csi_period 4096 a tile meets half the table."""
    for n_sym, n_rows, pad, pk, period in ((2047, 2, 1, "none", 52), (2048, 1, 0, "random", 4096), (2049, 3, 1, "reversal", 1),
                                           (6151, 2, 0, "none", 4096), (4100, 2, 1, "random", 52), (4097, 1, 1, "none", 0)):
        both_directions(api, order, n_sym, n_rows, pad, pk, period, seed=n_sym)


def test_more_workgroups_than_one_grid_row(api):
    """2^20 + 3 rows of one symbol: the call's workgroups fill one row of the grid and start the next."""
    n_rows = (1 << 20) + 3
    h = api.Qam(4, 1, 1.0, 1.0)
    z = qc.noisy_symbols(4, n_rows, 1, 1.0, 0.4, 1)
    d_z, d_o = sc.from_numpy(api, z.view(F32)), sc.device_array(api, 2 * n_rows)
    assert h.demap_stream(d_z, n_rows, d_o) == n_rows
    api.sync()
    got = d_o.to_numpy(keep=True)
    assert np.array_equal(_bits(got), _bits(api.qam_plan(4, 1, sym=z).ravel()))
    d_b, d_s = sc.from_bytes(api, np.arange(n_rows, dtype=np.uint32).astype(np.uint8)), sc.device_array(api, 2 * n_rows)
    assert h.map_stream(d_b, n_rows, d_s) == n_rows
    api.sync()
    want = api.qam_plan(4, 1, data=np.arange(n_rows, dtype=np.uint32).astype(np.uint8).reshape(-1, 1))
    assert np.array_equal(_bits(d_s.to_numpy(keep=True)), _bits(want.view(F32).ravel()))
    h.close()


# ---- the contracts about bits
@pytest.mark.parametrize("order", [2, 64, 256])
def test_runs_repeat_and_a_row_depends_on_itself_alone(api, order):
    """The same call twice; row 299 of 300 against the same row alone at another address, stride and alignment."""
    n_sym, n_rows = 257, 300
    B = n_sym * qc.BPS[order]
    perm = qc.perm_of("random", B, 3)
    idx, clen, csi = qc.csi_of(52, n_rows, 3)
    h = api.Qam(order, n_sym, 0.9, 1.5, perm, idx, clen)
    z = qc.noisy_symbols(order, n_rows, n_sym, 0.9, 0.4, 3)
    a = run_demap(api, h, z, csi, pad=1, lead=1)
    b = run_demap(api, h, z, csi, pad=1, lead=1)
    assert np.array_equal(_bits(a), _bits(b))
    for pad, lead in ((0, 0), (3, 2)):
        one = run_demap(api, h, z[299:], csi[299:], pad=pad, lead=lead, csi_pad=5)
        assert np.array_equal(_bits(one[0]), _bits(a[299])), (pad, lead)
    data = qc.coded_bytes(n_rows, h.n_bytes, 3)
    m = run_map(api, h, data, pad=1, lead=1)
    assert np.array_equal(_bits(m), _bits(run_map(api, h, data, pad=1, lead=1)))
    for pad, lead in ((0, 0), (3, 5)):
        assert np.array_equal(_bits(run_map(api, h, data[299:], pad=pad, lead=lead)[0]), _bits(m[299])), (pad, lead)
    h.close()


def test_the_exact_case_on_the_device(api):
    h = api.Qam(2, 1, 1.0, 1.0)
    r = h.demap(np.array([[0.5 + 0j]], np.complex64))
    assert r.shape == (1, 1) and _bits(r)[0, 0] == _bits(np.array([2.0], F32))[0]
    assert np.array_equal(_bits(h.map(np.array([[0x80]], np.uint8)).view(F32)), _bits(np.array([[-1.0, 0.0]], F32)))
    h.close()


# ---- refusals
def test_refusals_launch_nothing(api, L):
    order, n_sym, nr = 16, 10, 3
    idx, clen, csi = qc.csi_of(52, nr, 0)
    h = api.Qam(order, n_sym, csi_index=idx, csi_len=clen)
    hp = api.Qam(order, n_sym)                                       # no channel weighting
    B, nbytes = h.n_bits, h.n_bytes
    assert (B, nbytes, h.csi_period, h.csi_len, hp.csi_period) == (40, 5, 52, 64, 0)
    z = qc.noisy_symbols(order, nr, n_sym)
    data = qc.coded_bytes(nr, nbytes)
    d_z, d_h, d_b = sc.from_numpy(api, z.view(F32)), sc.from_numpy(api, csi.view(F32)), sc.from_bytes(api, data)
    d_o, d_s = sc.device_array(api, nr * B + 8), sc.device_array(api, 2 * nr * n_sym + 8)
    lib = L.load()
    k = C.c_size_t(7)

    def demap(pz=d_z.ptr, zs=n_sym, pc=d_h.ptr, cs=clen, n=nr, po=d_o.ptr, os_=B, hh=h._h, kk=C.byref(k)):
        return lib.sfe_dsp_qam_demap_stream(hh, pz, zs, pc, cs, n, po, os_, kk, None)

    def map_(pb=d_b.ptr, bs=nbytes, n=nr, po=d_s.ptr, os_=n_sym, hh=h._h, kk=C.byref(k)):
        return lib.sfe_dsp_qam_map_stream(hh, pb, bs, n, po, os_, kk, None)

    for why, rc in (("in_stride", demap(zs=n_sym - 1)), ("csi_stride", demap(cs=clen - 1)), ("out_stride", demap(os_=B - 1))):
        assert rc == L.SFE_ERANGE and lib.sfe_dsp_last_error().startswith(b"qam_demap_stream: "), why
    for why, rc in (("in_stride", map_(bs=nbytes - 1)), ("out_stride", map_(os_=n_sym - 1))):
        assert rc == L.SFE_ERANGE and lib.sfe_dsp_last_error().startswith(b"qam_map_stream: "), why
    for why, call in (("null symbols", lambda: demap(pz=None)), ("null csi on a csi handle", lambda: demap(pc=None)), ("null output", lambda: demap(po=None)),
                      ("csi on a handle without", lambda: demap(hh=hp._h)),
                      ("symbols off 8 bytes", lambda: demap(pz=d_z.ptr + 4, n=1)), ("csi off 8 bytes", lambda: demap(pc=d_h.ptr + 4, n=1)),
                      ("floats off 4 bytes", lambda: demap(po=d_o.ptr + 2)), ("2^31 rows", lambda: demap(n=1 << 31)),
                      ("a byte range to 2^62", lambda: demap(n=2, zs=1 << 59)), ("a csi range to 2^62", lambda: demap(n=2, cs=1 << 59)),
                      ("an output range to 2^62", lambda: demap(n=2, os_=1 << 60)),
                      ("the output over the symbols", lambda: demap(po=d_z.ptr + 8 * (nr * n_sym - 1))),
                      ("the output over the csi", lambda: demap(po=d_h.ptr + 8)), ("no count", lambda: demap(kk=None)), ("no handle", lambda: demap(hh=None))):
        assert call() == L.SFE_EINVAL and k.value == 0, why
        assert lib.sfe_dsp_last_error().startswith(b"qam_demap_stream: "), (why, lib.sfe_dsp_last_error())
    for why, call in (("null bytes", lambda: map_(pb=None)), ("null output", lambda: map_(po=None)), ("cf32 off 8 bytes", lambda: map_(po=d_s.ptr + 4)),
                      ("2^31 rows", lambda: map_(n=1 << 31)), ("a byte range to 2^62", lambda: map_(n=2, bs=1 << 62)),
                      ("an output range to 2^62", lambda: map_(n=2, os_=1 << 59)), ("the output over the bytes", lambda: map_(po=d_b.ptr + 8)),
                      ("no count", lambda: map_(kk=None)), ("no handle", lambda: map_(hh=None))):
        assert call() == L.SFE_EINVAL and k.value == 0, why
        assert lib.sfe_dsp_last_error().startswith(b"qam_map_stream: "), (why, lib.sfe_dsp_last_error())
    # a live handle of another block is refused, and qam's destroy frees nothing of it
    other = api.Corr(np.ones(13, np.complex64), 3840)
    assert demap(hh=other._h) == L.SFE_EINVAL and map_(hh=other._h) == L.SFE_EINVAL and k.value == 0
    assert lib.sfe_dsp_qam_destroy(other._h) == L.SFE_OK
    other.reset()
    other.close()
    with pytest.raises(AttributeError):
        h.reset()
    api.sync()
    assert (d_o.to_numpy(keep=True).view(np.uint32) == POISON).all() and (d_s.to_numpy(keep=True).view(np.uint32) == POISON).all()
    # no rows: a no-op, whatever the buffers
    assert demap(n=0, pz=None, pc=None, po=None) == L.SFE_OK and k.value == 0 and map_(n=0, pb=None, po=None) == L.SFE_OK and k.value == 0
    api.sync()
    assert (d_o.to_numpy(keep=True).view(np.uint32) == POISON).all() and (d_s.to_numpy(keep=True).view(np.uint32) == POISON).all()
    # the next good calls; coded bytes need no alignment
    assert demap() == L.SFE_OK and k.value == nr
    assert map_(pb=d_b.ptr + 1, n=2, bs=nbytes + 1) == L.SFE_OK and k.value == 2
    api.sync()
    assert np.array_equal(_bits(d_o.to_numpy(nr * B, keep=True)), _bits(api.qam_plan(order, n_sym, csi_index=idx, csi_len=clen, sym=z, csi=csi).ravel()))
    shifted = data.ravel()[1:][:2 * (nbytes + 1)].reshape(2, nbytes + 1)
    assert np.array_equal(_bits(d_s.to_numpy(4 * n_sym, keep=True)), _bits(api.qam_plan(order, n_sym, data=shifted).view(F32).ravel()))
    assert np.array_equal(_bits(h.demap(z, csi)), _bits(api.qam_plan(order, n_sym, csi_index=idx, csi_len=clen, sym=z, csi=csi)))
    assert np.array_equal(_bits(h.map(data).view(F32)), _bits(api.qam_plan(order, n_sym, data=data).view(F32)))
    h.close()
    hp.close()
    with pytest.raises(api.SfeError) as e:                           # a use after destroy: the wrapper holds no handle any more
        h.map_stream(d_b, nr, d_s)
    assert e.value.code == L.SFE_EINVAL


# ---- graph capture
def test_a_captured_call_replays_onto_a_poisoned_output(api, L):
    """Nothing in a handle changes after create: both calls are captured into one graph, replayed twice with the outputs
    poisoned again in between, and equal the eager calls' words each time."""
    hip = hip_runtime()
    order, n_sym, nr = 64, 257, 5
    B = n_sym * 6
    perm = qc.perm_of("random", B, 9)
    idx, clen, csi = qc.csi_of(52, nr, 9)
    h = api.Qam(order, n_sym, 1.0, 2.0, perm, idx, clen)
    z, data = qc.noisy_symbols(order, nr, n_sym, seed=9), qc.coded_bytes(nr, h.n_bytes, 9)
    eager_llr, eager_sym = run_demap(api, h, z, csi, pad=1, lead=1), run_map(api, h, data, pad=1, lead=1)
    assert np.array_equal(_bits(eager_llr), _bits(api.qam_plan(order, n_sym, 1.0, 2.0, perm, idx, clen, sym=z, csi=csi)))
    d_z, d_h = sc.from_numpy(api, lay(z, n_sym + 1, 1, np.complex64(0)).view(F32)), sc.from_numpy(api, csi.view(F32))
    d_b = sc.from_bytes(api, data)
    d_o, d_s = sc.device_array(api, 1 + nr * (B + 1) + 2), sc.device_array(api, 2 * (nr * (n_sym + 1) + 2))
    s, g, ex = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert hip.hipStreamCreate(C.byref(s)) == 0
    assert hip.hipStreamBeginCapture(s, 0) == 0
    try:
        k1 = h.demap_stream(d_z.ptr + 8, nr, d_o.ptr + 4, d_h, in_stride=n_sym + 1, out_stride=B + 1, stream=s.value)
        k2 = h.map_stream(d_b, nr, d_s, out_stride=n_sym + 1, stream=s.value)
    finally:
        ended = hip.hipStreamEndCapture(s, C.byref(g))
    assert ended == 0 and (k1, k2) == (nr, nr) and hip.hipGraphInstantiate(C.byref(ex), g, None, None, 0) == 0
    try:
        api.sync()
        assert (d_o.to_numpy(keep=True).view(np.uint32) == POISON).all()         # capturing ran nothing
        for _ in range(2):
            assert hip.hipGraphLaunch(ex, s) == 0 and hip.hipStreamSynchronize(s) == 0
            assert np.array_equal(taken(d_o, 1, nr, B, B + 1, 1), _bits(eager_llr))
            assert np.array_equal(taken(d_s, 2, nr, n_sym, n_sym + 1, 0), _bits(eager_sym))
            d_o.to_numpy(), d_s.to_numpy()                                       # reading without keep poisons them again
    finally:
        hip.hipGraphExecDestroy(ex)
        hip.hipGraphDestroy(g)
        hip.hipStreamDestroy(s)
        h.close()


# ---- the chain
def test_the_chain_on_the_device(api, L):
    """The CPU chain of tests/qam_cases.py at the same seed.  Transmit side: Ldpc.encode_stream -> Qam.map_stream ->
    OfdmMod.process_stream, each reading the block before it where its rows lie; the waveform equals the plans'.  The channel
    and the noise are the host's (they are no block).  Receive side: Ofdm (ZF) writes d_out and d_chan, Qam.demap_stream reads
    both as they lie and writes Ldpc's d_in: the payload bytes equal the input, and the demapper's soft values equal qam_plan's
    on the device's own Ofdm output."""
    c, o = qc.CHAIN, qc.chain()
    tx_args, rx_args, csi_index, perm = qc.chain_shapes()
    s, Z = lc.CASES["B"]
    a_, beta, max_iter = lc.PARAMS["a12"]
    nw, base, step, n_out = c["n_words"], o["starts"][0], o["starts"][1], o["n_out"]
    ldpc = api.Ldpc(s, Z, lc.SCALE, a_, beta, max_iter, in_mode=L.VIT_IN_SOFT)
    qam = api.Qam(c["order"], 162, 1.0, c["qam_scale"], perm, csi_index, 64)
    tx, rx = api.OfdmMod(**tx_args), api.Ofdm(**rx_args)
    assert (ldpc.n_bytes, qam.n_bytes, qam.n_sym, tx.n_in, rx.n_sym, qam.n_bits, ldpc.row) == (81, 81, 162, 162, 162, 648, 648)
    cstride, sstride, zstride, lstride = 84, 165, 163, 651           # rows a little apart, every second one off its 16-byte boundary
    d_pay = sc.from_bytes(api, o["pay"])
    d_code, d_sym, d_wave = sc.device_array(api, nw * cstride // 4), sc.device_array(api, 2 * nw * sstride), sc.device_array(api, 2 * n_out)
    assert ldpc.encode_stream(d_pay, nw, d_code, out_stride=cstride) == nw
    assert qam.map_stream(d_code, nw, d_sym, in_stride=cstride, out_stride=sstride) == nw
    assert tx.process_stream(d_sym, nw, d_wave, n_out, base, step, in_stride=sstride) == n_out
    api.sync()
    wave = d_wave.to_numpy(keep=True).view(np.complex64)
    assert mc.same(wave, o["wave"])
    x = qc.chain_channel(wave, qc.CHAIN_NOISE)
    assert mc.same(x, o["x"])
    d_x = sc.from_numpy(api, x.view(F32))
    d_z, d_ch, d_st = sc.device_array(api, 2 * nw * zstride), sc.device_array(api, 2 * nw * 64), sc.device_array(api, nw)
    d_llr, d_bits, d_rec, d_lst = sc.device_array(api, nw * lstride), sc.device_array(api, nw * 11), sc.device_array(api, 3 * nw), sc.device_array(api, nw)
    assert rx.process_stream(d_x, x.size, nw, d_z, d_chan=d_ch, d_status=d_st, start_base=base, start_step=step, out_stride=zstride) == nw
    assert qam.demap_stream(d_z, nw, d_llr, d_ch, in_stride=zstride, csi_stride=64, out_stride=lstride) == nw
    assert ldpc.process_stream(d_llr, nw, d_bits, d_rec, d_lst, d_status_in=d_st, in_stride=lstride, out_stride=44) == nw
    api.sync()
    z = d_z.to_numpy(keep=True).view(np.complex64).reshape(nw, zstride)[:, :162]
    ch = d_ch.to_numpy(keep=True).view(np.complex64).reshape(nw, 64)
    llr = taken(d_llr, 1, nw, 648, lstride, 0).view(F32)
    st, lst = d_st.to_numpy().view(np.int32), d_lst.to_numpy().view(np.int32)
    by = d_bits.to_numpy().view(np.uint8).reshape(nw, 44)[:, :41]
    print("receiver", st, "decoder", lst, "iterations", d_rec.to_numpy().view(np.uint32).reshape(nw, 3)[:, 0])
    for q in (ldpc, qam, tx, rx):
        q.close()
    assert not st.any() and not lst.any()
    assert np.array_equal(by, lc.payload_bits_only("B", o["pay"]))
    want = api.qam_plan(c["order"], 162, 1.0, c["qam_scale"], perm, csi_index, 64, sym=np.ascontiguousarray(z), csi=ch)
    assert np.array_equal(_bits(llr), _bits(want))
