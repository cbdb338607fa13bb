"""The Viterbi decoder (sfe_dsp_vit_*) on the GPU.  The bar is equality with api.vit_plan -- bytes, metric word, count and
status -- never a tolerance: every code, both endings, punctured and not, the launches above 64 KB of LDS and the one that
reads its soft values from global memory, the contracts about bits checked literally, a sentinel around every output of
every call, the refusals, a captured call, and the chain behind a real burst-demodulator handle."""
import ctypes as C

import numpy as np
import pytest

from simplefe_amd import synth
from vit_cases import SENT, rows_of, run, same

pytestmark = pytest.mark.gpu
F32 = np.float32
QNAN = 0x7fc00000
CODES = [(3, (7, 5)), (7, (0o171, 0o133)), (7, (0o133, 0o171, 0o165)), (8, (0o247, 0o371)), (9, (0o561, 0o753))]
CODE_IDS = ["K3", "K7", "K7n3", "K8", "K9"]
PUNCT = {2: [[1, 1], [1, 0], [0, 1]], 3: [[1, 1, 0], [1, 0, 0], [0, 0, 1]]}           # rate 3/4, period 3


@pytest.fixture(scope="module")
def api():
    from simplefe_amd import api as a
    return a


@pytest.fixture(scope="module")
def L():
    from simplefe_amd import lib
    return lib


@pytest.mark.parametrize("code", CODES, ids=CODE_IDS)
@pytest.mark.parametrize("terminated", [True, False], ids=["terminated", "truncated"])
def test_equality_with_the_plan(api, code, terminated):
    """Seven bursts per call -- noisy, integer-valued and all-zero rows -- at n_info 1, 5, 64 and 200, punctured and not."""
    K, gen = code
    for n_info in (1, 5, 64, 200):
        for keep in (None, PUNCT.get(len(gen))):
            x = rows_of(api, K, gen, n_info, keep, terminated, 7, 1000 * K + n_info)
            want = api.vit_plan(K, gen, n_info, keep, terminated, x=x)
            h = api.Vit(K, gen, n_info, keep, terminated)
            got = run(api, h, x, in_pad=n_info % 3, out_pad=n_info % 2, lead=1)
            h.close()
            assert not want[2].any() and not want[0][2].any() and want[1][2].tolist() == [0, 0]
            assert same(got, want), (n_info, keep)


# (K, gen, n_info, keep, terminated, staged): every one asks for more than 64 KB of LDS.  Staged:
# K = 7 at the longest burst (survivors 65 584 bytes, 132 192 in all), K = 8 (two states per lane) and K = 9 (four).  Not
# staged -- the soft values are read from global memory, 64 steps at a time: K = 9 at the last n_info create accepts, terminated
# and truncated (134 384 of the 134 400 bytes), K = 7 with three generators at the longest burst, punctured, and K = 9 with four.
G9 = (0o561, 0o753)
LARGE = [(7, (0o171, 0o133), 8192, None, True, True), (8, (0o247, 0o371), 5000, PUNCT[2], True, True), (9, G9, 2048, None, False, True),
         (9, G9, 4175, None, True, False), (9, G9, 4183, PUNCT[2], False, False), (7, (0o133, 0o171, 0o165), 8192, PUNCT[3], True, False),
         (9, (0o765, 0o671, 0o513, 0o473), 4000, None, False, False)]


@pytest.mark.parametrize("shape", LARGE, ids=["K7-8192", "K8-5000-punctured", "K9-2048", "K9-4175", "K9-4183-punctured", "K7n3-8192-punctured", "K9n4-4000"])
def test_large_footprints(api, shape):
    K, gen, n_info, keep, terminated, staged = shape
    base, is_staged, waves = api.vit_footprint(K, len(gen), n_info, terminated)
    assert base > 65536 and waves >= 1 and is_staged == staged
    x = rows_of(api, K, gen, n_info, keep, terminated, 3, 77 + K)
    want = api.vit_plan(K, gen, n_info, keep, terminated, x=x)
    h = api.Vit(K, gen, n_info, keep, terminated)
    got = run(api, h, x, in_pad=1, out_pad=3)
    h.close()
    assert not want[2].any() and same(got, want)


@pytest.mark.parametrize("code", [CODES[1], CODES[3]], ids=[CODE_IDS[1], CODE_IDS[3]])
def test_runs_repeat_and_a_burst_depends_on_its_values_alone(api, code):
    """The same call twice; every burst of a 70-burst call against a one-burst call at another address and other strides."""
    K, gen = code
    n_info, keep = 61, PUNCT[2]
    x = rows_of(api, K, gen, n_info, keep, True, 70, 5)
    h = api.Vit(K, gen, n_info, keep)
    a = run(api, h, x, in_pad=3, out_pad=1, lead=2)
    b = run(api, h, x, in_pad=3, out_pad=1, lead=2)
    assert same(a, b) and same(a, api.vit_plan(K, gen, n_info, keep, x=x))
    for i in range(70):
        one = run(api, h, x[i:i + 1], in_pad=i % 4, out_pad=i % 5, lead=1 + i % 3)
        assert same(one, [v[i:i + 1] for v in a]), i
    h.close()


@pytest.mark.parametrize("code", [CODES[1], CODES[4]], ids=[CODE_IDS[1], CODE_IDS[4]])
def test_symbol_input_gives_the_bits_of_soft_input(api, L, code):
    """BPSK and QPSK rows -- what is not read is NaN or infinite -- against SOFT rows of the extracted components."""
    K, gen = code
    n_info, skip = 45, 3
    x = rows_of(api, K, gen, n_info, None, True, 5, 9)
    n_soft = x.shape[1]
    h = api.Vit(K, gen, n_info)
    want = run(api, h, x)
    h.close()
    assert not want[2].any()
    bp = np.full((5, skip + n_soft + 2), np.nan + 0j, np.complex64)
    bp[:, skip:skip + n_soft].real = x
    bp[:, skip:skip + n_soft].imag = np.inf
    h = api.Vit(K, gen, n_info, in_mode=L.VIT_IN_BPSK, skip=skip)
    assert same(run(api, h, bp, in_pad=1, lead=1), want)
    h.close()
    qp = np.full((5, skip + n_soft // 2 + 1), np.nan + 0j, np.complex64)
    qp[:, skip:skip + n_soft // 2] = x[:, 0::2] + 1j * x[:, 1::2]
    h = api.Vit(K, gen, n_info, in_mode=L.VIT_IN_QPSK, skip=skip)
    assert same(run(api, h, qp, in_pad=2, lead=3), want)
    h.close()


@pytest.mark.parametrize("shape", [(7, (0o171, 0o133), 100, PUNCT[2]), (7, (0o133, 0o171, 0o165), 8192, None)], ids=["staged", "unstaged"])
def test_failed_bursts_get_the_stated_bits_and_leave_their_neighbours_alone(api, shape):
    """Of six bursts one holds a NaN as its first value and one an infinity as its last, and a third has a nonzero word in
    the status table -- its row is NaN throughout and is not read; the rest equal a call without any of that."""
    K, gen, n_info, keep = shape
    x = rows_of(api, K, gen, n_info, keep, True, 6, 21)
    h = api.Vit(K, gen, n_info, keep)
    clean = run(api, h, x)
    bad = x.copy()
    bad[1, 0] = np.nan
    bad[3, -1] = -np.inf
    bad[4, :] = np.nan
    got = run(api, h, bad, status_in=[0, 0, 0, 0, 7, 0])
    h.close()
    assert not clean[2].any() and got[2].tolist() == [0, 1, 0, 1, 2, 0]
    assert same(got, api.vit_plan(K, gen, n_info, keep, x=bad, status_in=[0, 0, 0, 0, 7, 0]))
    for b in range(6):
        if got[2][b]:
            assert not got[0][b].any() and got[1][b].tolist() == [QNAN, 0]
        else:
            assert np.array_equal(got[0][b], clean[0][b]) and np.array_equal(got[1][b], clean[1][b])


def test_a_captured_call_replays(api):
    """Nothing in a handle changes after create, so a call under graph capture is supported: the replayed node's output
    equals the plan's."""
    hip = C.CDLL("libamdhip64.so")
    for name, args in (("hipStreamCreate", [C.POINTER(C.c_void_p)]), ("hipStreamBeginCapture", [C.c_void_p, C.c_int]),
                       ("hipStreamEndCapture", [C.c_void_p, C.POINTER(C.c_void_p)]),
                       ("hipGraphInstantiate", [C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
                       ("hipGraphLaunch", [C.c_void_p, C.c_void_p]), ("hipStreamSynchronize", [C.c_void_p]),
                       ("hipGraphExecDestroy", [C.c_void_p]), ("hipGraphDestroy", [C.c_void_p]), ("hipStreamDestroy", [C.c_void_p])):
        fn = getattr(hip, name)
        fn.argtypes, fn.restype = args, C.c_int
    K, gen, n_info = 7, (0o171, 0o133), 200
    x = rows_of(api, K, gen, n_info, None, True, 9, 31)
    h = api.Vit(K, gen, n_info)

    def captured(*args, **kw):
        s, g, ex = C.c_void_p(), C.c_void_p(), C.c_void_p()
        assert hip.hipStreamCreate(C.byref(s)) == 0
        assert hip.hipStreamBeginCapture(s, 0) == 0
        try:
            k = h.process_stream(*args, stream=s.value, **kw)
        finally:
            ended = hip.hipStreamEndCapture(s, C.byref(g))
        assert ended == 0 and hip.hipGraphInstantiate(C.byref(ex), g, None, None, 0) == 0
        try:
            assert hip.hipGraphLaunch(ex, s) == 0 and hip.hipStreamSynchronize(s) == 0
        finally:
            hip.hipGraphExecDestroy(ex)
            hip.hipGraphDestroy(g)
            hip.hipStreamDestroy(s)
        return k

    got = run(api, h, x, in_pad=1, out_pad=2, call=captured)
    h.close()
    assert same(got, api.vit_plan(K, gen, n_info, x=x))


def test_refusals_launch_nothing(api, L):
    K, gen, n_info, nb = 7, (0o171, 0o133), 64, 3
    h = api.Vit(K, gen, n_info)
    n_soft, nbytes = h.n_soft, h.n_bytes
    assert (n_soft, nbytes) == (140, 8)
    x = rows_of(api, K, gen, n_info, None, True, nb, 41)
    d_in = api.DeviceArray.from_numpy(np.concatenate([x.ravel(), np.zeros(64, F32)]))
    sentinel = np.full(256, SENT, F32)
    d_by, d_rec, d_st, d_si = (api.DeviceArray.from_numpy(sentinel) for _ in range(4))
    d_si.zero()
    lib = L.load()
    k = C.c_size_t(7)

    def call(pi=d_in.ptr, istride=n_soft, psi=d_si.ptr, n_bursts=nb, pb=d_by.ptr, ostride=nbytes, pr=d_rec.ptr, ps=d_st.ptr, hh=None, kk=C.byref(k)):
        return lib.sfe_dsp_vit_process_stream(hh or h._h, pi, istride, psi, n_bursts, pb, ostride, pr, ps, kk, None)

    assert call(istride=n_soft - 1) == L.SFE_ERANGE and lib.sfe_dsp_last_error().startswith(b"vit_process_stream: ")
    assert call(ostride=nbytes - 1) == L.SFE_ERANGE
    assert call(pi=None) == L.SFE_EINVAL and call(pb=None) == L.SFE_EINVAL
    assert call(pi=d_in.ptr + 2) == L.SFE_EINVAL                     # misaligned, each of the four-byte buffers
    assert call(psi=d_si.ptr + 1) == L.SFE_EINVAL
    assert call(pr=d_rec.ptr + 2) == L.SFE_EINVAL
    assert call(ps=d_st.ptr + 3) == L.SFE_EINVAL
    assert call(n_bursts=1 << 31) == L.SFE_EINVAL
    assert call(istride=1 << 61) == L.SFE_EINVAL and call(ostride=1 << 62) == L.SFE_EINVAL       # byte ranges that reach 2^62
    assert call(pb=d_in.ptr + 4 * (nb * n_soft) - 1) == L.SFE_EINVAL  # each output over the input and over the status table
    assert call(pr=d_in.ptr) == L.SFE_EINVAL and call(ps=d_in.ptr + 8) == L.SFE_EINVAL
    assert call(pb=d_si.ptr + 4 * nb - 1) == L.SFE_EINVAL and call(pr=d_si.ptr + 4) == L.SFE_EINVAL and call(ps=d_si.ptr) == L.SFE_EINVAL
    assert call(pr=d_by.ptr + 8) == L.SFE_EINVAL                     # two outputs over one another
    assert call(ps=d_by.ptr + 4 * ((nb * nbytes - 1) // 4)) == L.SFE_EINVAL
    assert call(ps=d_rec.ptr + 4) == L.SFE_EINVAL
    assert call(kk=None) == L.SFE_EINVAL
    assert k.value == 0
    assert call(n_bursts=0) == L.SFE_OK and k.value == 0             # no bursts: a no-op
    # symbol rows are eight-byte aligned and skip + n_soft symbols long
    hb = api.Vit(K, gen, n_info, in_mode=L.VIT_IN_BPSK, skip=4)
    assert call(hh=hb._h, pi=d_in.ptr + 4, istride=4 + n_soft) == L.SFE_EINVAL
    assert call(hh=hb._h, istride=4 + n_soft - 1) == L.SFE_ERANGE
    hb.close()
    # a live handle of another block is refused, and vit's destroy frees nothing of it
    other = api.Corr(np.ones(13, np.complex64), 3840)
    assert call(hh=other._h) == L.SFE_EINVAL and k.value == 0
    assert lib.sfe_dsp_vit_destroy(other._h) == L.SFE_OK
    other.reset()                                                    # still alive
    other.close()
    with pytest.raises(AttributeError):
        h.reset()
    api.sync()
    for d in (d_by, d_rec, d_st):
        assert np.array_equal(d.to_numpy().view(np.uint32), sentinel.view(np.uint32))
    # the next good call is a fresh handle's; the optional buffers may be left out
    want = api.vit_plan(K, gen, n_info, x=x)
    assert call() == L.SFE_OK and k.value == nb
    assert call(psi=None, pr=None, ps=None) == L.SFE_OK and k.value == nb
    api.sync()
    assert np.array_equal(d_by.to_numpy().view(np.uint8)[:nb * nbytes].reshape(nb, nbytes), want[0])
    assert np.array_equal(d_rec.to_numpy(2 * nb).view(np.uint32).reshape(nb, 2), want[1])
    assert not d_st.to_numpy(nb).view(np.int32).any()
    assert same(h.decode(x), want)
    h.close()
    for d in (d_in, d_by, d_rec, d_st, d_si):
        d.free()


# the chain's shape: (sps, N) = (10, 256), a 32-symbol QPSK preamble, then the 224 coded bits of 106 payload bits as BPSK
CHAIN = dict(sps=10, N=256, Lp=32, lag=4, K=7, gen=(0o171, 0o133), n_info=106)


def chain_signal(api):
    """Four noise-free bursts of different payloads, timings, carriers and amplitudes, one window each: (x, the preamble,
    the payloads' bytes, the window's length).  tests/test_vit_host.py's law and the burst plan decode all four on the CPU."""
    c = CHAIN
    pre = synth.psk_symbols(c["Lp"], 4, seed=synth.SEED + 3)
    win = (c["N"] + 2) * c["sps"] + 30
    xs, want = [], []
    for b, (tau, f, phase, amp) in enumerate([(0.3, 0.002, 0.4, 0.8), (-1.25, -0.003, -2.0, 1.7), (0.0, 0.001, 1.0, 1.0), (2.2, 0.0, 2.5, 0.4)]):
        bits = synth.vit_bits(c["n_info"], 500 + b)
        sym = np.concatenate([pre, synth.vit_symbols(api.vit_encode(c["K"], c["gen"], bits), 2)])
        assert sym.size == c["N"]
        xs.append(synth.burst_signal(sym, c["sps"], win, c["sps"] + 7, tau, f, phase, amp))
        want.append(synth.vit_pack(bits))
    return np.concatenate(xs), pre.astype(np.complex64), np.stack(want), win


def test_the_chain_behind_a_burst_demodulator_stays_on_the_device(api, L):
    """A real Burst handle writes symbols and statuses; Vit reads its d_out, out_stride, skip = Lp and status table as they
    lie.  Burst 2 is gated off and arrives as status 2; the decoded bytes of the others are the transmitted ones, and they
    are the plan's on the device's own symbols."""
    c = CHAIN
    x, pre, want, win = chain_signal(api)
    # on the CPU first: the plan on the burst plan's symbols decodes every burst
    psym = api.burst_plan(pre, c["sps"], c["N"], c["lag"], x=x, n_bursts=4, start_base=c["sps"] + 7, start_step=win)[0]
    assert np.array_equal(api.vit_plan(c["K"], c["gen"], c["n_info"], in_mode=L.VIT_IN_BPSK, skip=c["Lp"], x=psym)[0], want)
    hb = api.Burst(pre, c["sps"], c["N"], c["lag"], min_gate=0.5)
    hv = api.Vit(c["K"], c["gen"], c["n_info"], in_mode=L.VIT_IN_BPSK, skip=c["Lp"])
    d_x, d_gate = api.DeviceArray.from_numpy(x.view(F32)), api.DeviceArray.from_numpy(np.array([1, 1, 0.25, 1], F32))
    d_sym, d_brec, d_bst = api.DeviceArray(4 * c["N"] * 2), api.DeviceArray(4 * 8), api.DeviceArray(4)
    d_by, d_rec, d_st = api.DeviceArray((4 * hv.n_bytes + 3) // 4), api.DeviceArray(8), api.DeviceArray(4)
    try:
        assert hb.process_stream(d_x, x.size, 4, d_sym, None, d_gate, d_brec, d_bst, start_base=c["sps"] + 7, start_step=win) == 4
        assert hv.process_stream(d_sym, 4, d_by, d_rec, d_st, d_bst, in_stride=c["N"]) == 4
        api.sync()
        sym = d_sym.to_numpy().view(np.complex64).reshape(4, c["N"])
        by = d_by.to_numpy().view(np.uint8)[:4 * hv.n_bytes].reshape(4, hv.n_bytes)
        rec, st, bst = d_rec.to_numpy().view(np.uint32).reshape(4, 2), d_st.to_numpy().view(np.int32), d_bst.to_numpy().view(np.int32)
    finally:
        for d in (d_x, d_gate, d_sym, d_brec, d_bst, d_by, d_rec, d_st):
            d.free()
        hb.close()
        hv.close()
    print("burst statuses", bst, "vit statuses", st, "metrics", rec[:, 0].copy().view(F32), "counts", rec[:, 1])
    assert bst.tolist() == [0, 0, 2, 0] and st.tolist() == [0, 0, 2, 0]
    for b in (0, 1, 3):
        assert np.array_equal(by[b], want[b]) and rec[b, 1] == 0
    assert not by[2].any() and rec[2].tolist() == [QNAN, 0]
    assert same((by, rec, st), api.vit_plan(c["K"], c["gen"], c["n_info"], in_mode=L.VIT_IN_BPSK, skip=c["Lp"], x=sym, status_in=bst))
