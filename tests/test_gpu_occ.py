"""The spectrum occupancy detector on the GPU (sfe_dsp_occ_*, csrc/occ.hip).  The bar is equality with the host plan
(api.occ_plan, the same law compiled for the host; tests/test_occ_host.py holds the plan to the numpy restatement of the
law) -- bytes, never a tolerance.  Every call reads rows that sit at an offset inside a buffer of NaN poison, with a gap
between the streams, and writes info, records and mask into three buffers that are poisoned before the call and sit
between guards, with out_stride > n_rows (the layouts and verdicts of tests/stream_checks.py): exactly the call's slots
lose their poison, every byte of them, and nothing else changes.  `-m gpu`."""
import ctypes as C
import os

import numpy as np
import pytest

import occ_cases as oc
import stream_checks as sc
from simplefe_amd import synth

pytestmark = pytest.mark.gpu
CASES = oc.constructed()


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


def same_bytes(got, want, what):
    for name, g, w in zip(("info", "rec", "mask"), got, want):
        if g is None:
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.shape, w.shape)
        gb, wb = np.ascontiguousarray(g).view(np.uint8).reshape(-1), np.ascontiguousarray(w).view(np.uint8).reshape(-1)
        d = gb != wb
        if d.any():
            i = int(np.flatnonzero(d)[0])
            row = i // (gb.size // g.shape[0])
            raise AssertionError("%s: %s differs in %d bytes, the first in row %d: %r != %r" % (what, name, int(d.sum()), row, g[row], w[row]))


def run_occ(api, h, rows, with_mask=True, lead=64, in_gap=7, out_gap=3):
    """Occ.process_stream through poisoned, guarded buffers: rows (n_streams, n_rows, N) float32.  The input starts `lead`
    bytes into a buffer of poison (a NaN) with in_gap floats between the streams; each output has a front guard, out_gap
    slots between the streams and a tail guard.  Returns (info (S*J,), rec (S*J, E), mask (S*J, N) or None)."""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    S, J, N = rows.shape
    E = h.max_emissions
    ilay = sc.Layout(S, 4, J * N, J * N + in_gap, lead, 64)
    iraw = ilay.poisoned()
    for s in range(S):
        ilay.put(iraw, s, rows[s])
    so = J + out_gap
    lays = [sc.Layout(S, 16, J, so, 256, 256), sc.Layout(S, 32 * E, J, so, 256, 256), sc.Layout(S, N, J, so, 256, 256)]
    if not with_mask:
        lays = lays[:2]
    d_in = api.DeviceArray.from_numpy(iraw.view(np.float32))
    d_out = [api.DeviceArray.from_numpy(l.poisoned().view(np.float32)) for l in lays]
    try:
        k = h.process_stream(d_in.ptr + ilay.front, J, d_out[0].ptr + 256, d_out[1].ptr + 256, d_out[2].ptr + 256 if with_mask else None,
                             n_streams=S, in_stride=ilay.stride_items, out_stride=so)
        api.sync()
        raws = [d.to_numpy().view(np.uint32) for d in d_out]
        iafter = d_in.to_numpy().view(np.uint32)
    finally:
        d_in.free()
        for d in d_out:
            d.free()
    if k != S * J:
        raise sc.CountError("%d x %d rows: n_done %d" % (S, J, k))
    for raw, lay in zip(raws, lays):
        sc.check_written(raw, lay, J)
    sc.check_input_intact(iafter, iraw)
    info = np.concatenate([lays[0].take(raws[0], s, J, synth.OCC_INFO) for s in range(S)])
    rec = np.concatenate([lays[1].take(raws[1], s, J, synth.OCC_REC).reshape(J, E) for s in range(S)])
    mask = np.concatenate([lays[2].take(raws[2], s, J, np.uint8).reshape(J, N) for s in range(S)]) if with_mask else None
    return info, rec, mask


def make(api, N, p):
    return api.Occ(N, p["rank"], p["factor"], p["min_level"], p["gap"], p["min_width"], p["max_emissions"], p["shift"])


# ------------------------------------------------------------------------------------------------ the plan's bytes
@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (2, 257)], ids=["1x1", "3x5", "2x257"])
@pytest.mark.parametrize("N", [16, 250, 256, 1024, 4096])
def test_the_device_gives_the_plans_bytes(api, N, shape):
    S, J = shape
    rows = oc.random_rows(N, S * J, seed=7 * N + J)
    if S * J > 4:
        rows[2, N // 3] = np.nan                    # one non-finite row among its neighbours
    emissions = 0
    for k, base in enumerate(oc.SETS):
        p = oc.params(N, **base)
        want = api.occ_plan(rows, **p)
        emissions += int(want[0]["count"].sum())
        h = make(api, N, p)
        for with_mask in (True, False):
            got = run_occ(api, h, rows.reshape(S, J, N), with_mask, lead=64 + 4 * ((k + J) % 4))
            same_bytes(got, want, "N %d, %d x %d rows, set %d, %s mask" % (N, S, J, k, "with" if with_mask else "without"))
        h.close()
    assert emissions > 0


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_the_constructed_rows(api, case):
    name, rows, p, check = case
    N = rows.shape[1]
    h = make(api, N, p)
    got = run_occ(api, h, rows[None], True)
    same_bytes(got, api.occ_plan(rows, **p), name)
    check(*got)
    same_bytes(run_occ(api, h, rows[:, None], False, lead=68), got, name + ", a stream per row, no mask")
    h.close()


# ------------------------------------------------------------------------------------------------ the contracts about bits
@pytest.mark.parametrize("N", [250, 1024])
def test_a_rows_outputs_depend_on_that_row_alone(api, N):
    S, J = 3, 5
    rows = oc.random_rows(N, S * J, seed=N + 1)
    rows[7] = rows[0]                               # the same row twice: the same bytes twice
    p = oc.params(N, **oc.SETS[0])
    h = make(api, N, p)
    all_ = run_occ(api, h, rows.reshape(S, J, N))
    same_bytes(all_, api.occ_plan(rows, **p), "3 x 5 rows")
    for i in range(S * J):
        one = run_occ(api, h, rows[i].reshape(1, 1, N), lead=64 + 4 * (i % 4), out_gap=1 + i % 3)
        same_bytes(one, tuple(a[i:i + 1] for a in all_), "row %d alone" % i)
    for a in all_:
        assert a[7].tobytes() == a[0].tobytes()
    # other strides, another address, the streams cut differently: the same rows, the same bytes
    moved = run_occ(api, h, rows.reshape(5, 3, N), lead=76, in_gap=N + 1, out_gap=11)
    same_bytes(moved, all_, "5 x 3 rows at other strides")
    same_bytes(run_occ(api, h, rows.reshape(1, 15, N), lead=64, in_gap=0, out_gap=0), all_, "1 x 15 rows")
    h.close()


# ------------------------------------------------------------------------------------------------ capture
class Hip:
    """The HIP graph calls a capturing caller makes, through libamdhip64 (the product library is not involved)."""

    def __init__(self):
        self.h = C.CDLL("libamdhip64.so")
        vp, pvp = C.c_void_p, C.POINTER(C.c_void_p)
        for name, args in (("hipStreamCreate", [pvp]), ("hipStreamBeginCapture", [vp, C.c_int]), ("hipStreamEndCapture", [vp, pvp]),
                           ("hipGraphInstantiate", [pvp, vp, vp, vp, C.c_size_t]), ("hipGraphLaunch", [vp, vp]),
                           ("hipStreamSynchronize", [vp]), ("hipGraphExecDestroy", [vp]), ("hipGraphDestroy", [vp]),
                           ("hipStreamDestroy", [vp]), ("hipGraphGetNodes", [vp, pvp, C.POINTER(C.c_size_t)])):
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

    def nodes(self, g):
        n = C.c_size_t(0)
        self.ok(self.h.hipGraphGetNodes(g, None, C.byref(n)))
        return n.value

    def free(self, s, g, ex):
        self.h.hipGraphExecDestroy(ex)
        self.h.hipGraphDestroy(g)
        self.h.hipStreamDestroy(s)


def test_a_captured_call_replays_on_new_contents(api, L):
    env = dict(os.environ)
    hip = Hip()
    S, J, N, E = 2, 3, 1024, 16
    si, so = J * N + 4, J + 2
    p = oc.params(N, **oc.SETS[0])
    h = make(api, N, p)
    chunks = [oc.random_rows(N, S * J, seed=40 + i) for i in range(5)]
    d_in = sc.device_array(api, S * si)
    d_info, d_rec, d_mask = sc.device_array(api, 4 * S * so), sc.device_array(api, 8 * E * S * so), sc.device_array(api, N * S * so // 4)

    def put(i, stream=None):
        pad = np.zeros((S, si), np.float32)
        pad[:, :J * N] = chunks[i].reshape(S, J * N)
        api.check(L.load().sfe_dsp_memcpy_h2d(d_in.ptr, pad.ctypes.data, pad.nbytes, stream))
        api.check(L.load().sfe_dsp_sync(stream))

    def call(stream=None):
        return h.process_stream(d_in.ptr, J, d_info.ptr, d_rec.ptr, d_mask.ptr, n_streams=S, in_stride=si, out_stride=so, stream=stream)

    def take(i, what, stream=None):
        info = d_info.to_numpy(stream=stream).view(synth.OCC_INFO).reshape(S, so)
        rec = d_rec.to_numpy(stream=stream).view(synth.OCC_REC).reshape(S, so, E)
        mask = d_mask.to_numpy(stream=stream).view(np.uint8).reshape(S, so, N)
        got = (info[:, :J].reshape(-1), rec[:, :J].reshape(-1, E), mask[:, :J].reshape(-1, N))
        same_bytes(got, api.occ_plan(chunks[i], **p), what)
        for a in (info, rec, mask):                              # the slots between the streams' rows
            assert (np.ascontiguousarray(a[:, J:]).view(np.uint32) == sc.POISON).all(), what

    put(0)
    assert call() == S * J
    api.sync()
    take(0, "the eager call before the capture")
    ks = []
    s, g, ex = hip.capture(lambda st: ks.append(call(st)))
    assert ks == [S * J] and hip.nodes(g) == 1                   # one kernel launch, nothing else
    for i, kind in ((1, "g"), (2, "g"), (3, "e"), (4, "g")):
        if kind == "g":
            put(i, s.value)
            hip.ok(hip.h.hipGraphLaunch(ex, s))
            hip.ok(hip.h.hipStreamSynchronize(s))
            take(i, "replay on chunk %d" % i, s.value)
        else:
            put(i)
            assert call() == S * J
            api.sync()
            take(i, "the eager call between the replays")
    hip.free(s, g, ex)
    h.close()
    assert dict(os.environ) == env


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_launch_nothing(api, L):
    lib = L.load()
    S, J, N, E = 2, 4, 256, 16
    p = oc.params(N, **oc.SETS[0])
    rows = oc.random_rows(N, S * J, seed=3)
    d_in = sc.from_numpy(api, np.concatenate([rows.ravel(), np.zeros(64, np.float32)]))
    d_info, d_rec, d_mask = sc.device_array(api, 4 * S * J), sc.device_array(api, 8 * E * S * J), sc.device_array(api, N * S * J // 4)
    h = make(api, N, p)
    k = C.c_size_t(7)

    def call(pi, n_streams, n_rows, in_stride, pinfo, prec, pmask, out_stride):
        k.value = 7
        rc = lib.sfe_dsp_occ_process_stream(h._h, pi, n_streams, n_rows, in_stride, pinfo, prec, pmask, out_stride, C.byref(k), None)
        if rc != L.SFE_OK:
            assert k.value == 0 and lib.sfe_dsp_last_error().startswith(b"occ_process_stream: "), lib.sfe_dsp_last_error()
        return rc

    i, f, r, m = d_in.ptr, d_info.ptr, d_rec.ptr, d_mask.ptr
    assert call(i + 2, S, J, J * N, f, r, m, J) == L.SFE_EINVAL                   # float32 wants 4 bytes
    assert call(i, S, J, J * N, f + 2, r, m, J) == L.SFE_EINVAL
    assert call(i, S, J, J * N, f, r + 1, m, J) == L.SFE_EINVAL
    assert call(i, S, J, J * N, f, r, m, J - 1) == L.SFE_ERANGE                   # out_stride one slot short
    assert call(i, S, J, J * N - 1, f, r, m, J) == L.SFE_EINVAL                   # in_stride short with two streams
    assert call(None, S, J, J * N, f, r, m, J) == L.SFE_EINVAL
    assert call(i, S, J, J * N, None, r, m, J) == L.SFE_EINVAL
    assert call(i, S, J, J * N, f, None, m, J) == L.SFE_EINVAL
    assert call(i, S, J, J * N, i + 4 * S * J * N - 4, r, m, J) == L.SFE_EINVAL   # info over the input's last word
    assert call(i, S, J, J * N, f, i + 64, m, J) == L.SFE_EINVAL                  # the records inside the input
    assert call(i, S, J, J * N, f, r, i + 1, J) == L.SFE_EINVAL                   # the mask inside the input
    assert call(i, S, J, J * N, f, f + 16, m, J) == L.SFE_EINVAL                  # two outputs overlap
    assert call(i, S, J, J * N, f, r, r + 32 * E * S * J - 1, J) == L.SFE_EINVAL  # the mask over the records' last byte
    assert call(i, S, J, J * N, f, r, f + 16 * S * J - 1, J) == L.SFE_EINVAL
    assert call(i, 1 << 16, 1 << 15, J * N, f, r, m, 1 << 15) == L.SFE_EINVAL     # 2^31 rows
    assert call(i, 1, 1 << 31, J * N, f, r, m, 1 << 31) == L.SFE_EINVAL
    assert call(i, S, J, 1 << 62, f, r, m, J) == L.SFE_EINVAL                     # a stride that leaves the address space
    assert call(i, 0, J, J * N, f, r, m, J) == L.SFE_OK and k.value == 0          # no streams, no rows: no-ops, null buffers too
    assert call(None, S, 0, 0, None, None, None, 0) == L.SFE_OK and k.value == 0
    api.sync()
    for d in (d_info, d_rec, d_mask):
        assert (d.to_numpy(keep=True).view(np.uint32) == sc.POISON).all()         # nothing was stored; check_guarded holds the rest
    assert call(i, S, J, J * N, f, r, m, J) == L.SFE_OK and k.value == S * J
    api.sync()
    got = (d_info.to_numpy().view(synth.OCC_INFO), d_rec.to_numpy().view(synth.OCC_REC).reshape(-1, E), d_mask.to_numpy().view(np.uint8).reshape(-1, N))
    same_bytes(got, api.occ_plan(rows, **p), "after the refusals")
    with pytest.raises(AttributeError):
        h.reset()
    h.close()


# ------------------------------------------------------------------------------------------------ behind the spectrum estimator
def test_psd_rows_are_read_in_place(api):
    """Psd -> Occ on the device.  N = 1024, hop N, A = 16, a periodic Hann window, scale 1 / (A sum w^2); unit-variance complex
    Gaussian noise plus four on-bin tones of amplitude 0.5.  A tone puts N/6 = 171 into its bin and a quarter of that into
    each neighbour (the periodic Hann window leaks no further), against a floor near 0.83 and a factor of 8.  The largest
    noise bin the CPU step measures here is 2.61 x the floor (seed 0: 2.61, 2.37, 2.45, 2.55 for the four rows), so the factor
    is more than twice the largest noise-to-floor ratio; the test holds it to that."""
    N, A, S, J = 1024, 16, 2, 2
    tones = [-507, -128, 3, 257]
    w = (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(N) / N)).astype(np.float32)
    scale = np.float32(1.0 / (A * np.sum(w.astype(np.float64) ** 2)))
    n = J * A * N
    x = []
    for s in range(S):
        rng = np.random.default_rng(s)
        v = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2.0)
        for b in tones:
            v = v + 0.5 * np.exp(2j * np.pi * b * np.arange(n) / N)
        x.append(v.astype(np.complex64))
    x = np.stack(x)
    p = dict(rank=N // 4, factor=8.0, min_level=0.0, gap=2, min_width=1, max_emissions=16, shift=True)
    want = [(b - 1, b + 1, b) for b in tones]

    def four(info, rec, what):
        assert (info["count"] == 4).all() and (info["status"] == 0).all(), (what, info)
        for r in rec:
            assert [(int(e["lo"]), int(e["hi"]), int(e["peak"])) for e in r[:4]] == want, (what, r[:4])

    # on the CPU, from the float64 reference: the law finds exactly the four tones, with room
    ref = np.stack([synth.psd_reference(x[s], w, N, A, scale) for s in range(S)]).reshape(S * J, N)
    info, rec, _ = synth.occ_reference(ref.astype(np.float32), **p)
    four(info, rec, "the float64 reference's rows")
    quiet = np.ones(N, bool)
    quiet[[(b + d) % N for b in tones for d in (-1, 0, 1)]] = False
    ratio = max(float(r[quiet].max() / np.sort(r)[N // 4]) for r in ref)
    print("largest noise bin / floor: %.3f" % ratio)
    assert p["factor"] >= 2.0 * ratio

    ps = api.Psd(w, N, A, scale=float(scale), n_streams=S)
    oc_ = api.Occ(N, **p)
    d_x = sc.from_numpy(api, x.view(np.float32))
    stride, so = J * N + 8, J + 1
    d_rows = sc.device_array(api, S * stride)
    d_info, d_rec, d_mask = sc.device_array(api, 4 * S * so), sc.device_array(api, 8 * 16 * S * so), sc.device_array(api, N * S * so // 4)
    assert ps.process_stream(d_x.ptr, n, d_rows.ptr, out_stride=stride) == J
    assert oc_.process_stream(d_rows.ptr, J, d_info.ptr, d_rec.ptr, d_mask.ptr, n_streams=S, in_stride=stride, out_stride=so) == S * J
    api.sync()
    rows = d_rows.to_numpy(keep=True).reshape(S, stride)
    assert (rows[:, J * N:].view(np.uint32) == sc.POISON).all()
    rows = np.ascontiguousarray(rows[:, :J * N]).reshape(S * J, N)
    info = d_info.to_numpy().view(synth.OCC_INFO).reshape(S, so)
    rec = d_rec.to_numpy().view(synth.OCC_REC).reshape(S, so, 16)
    mask = d_mask.to_numpy().view(np.uint8).reshape(S, so, N)
    for a in (info, rec, mask):
        assert (np.ascontiguousarray(a[:, J:]).view(np.uint32) == sc.POISON).all()
    got = (info[:, :J].reshape(-1), rec[:, :J].reshape(-1, 16), mask[:, :J].reshape(-1, N))
    four(got[0], got[1], "the device's records from the device's rows")
    same_bytes(got, api.occ_plan(rows, **p), "the device against the plan on the device's rows")
    own = sorted((b + d) % N for b in tones for d in (-1, 0, 1))
    assert all(sorted(np.flatnonzero(m)) == own for m in got[2])          # the mask gates channels in psd's own numbering
    # the detector changed nothing it read
    assert np.array_equal(d_rows.to_numpy(keep=True).reshape(S, stride)[:, :J * N].reshape(S * J, N).view(np.uint32), rows.view(np.uint32))
    ps.close()
    oc_.close()
