"""The FIR, integer-step and general-rate kernels at the smallest shapes that reach each family, through the runners of
tests/stream_checks.py: the output poisoned before every call and guarded in front, behind and between channels, NaN
beside every input, the input read back and compared, counts equal to the reference's call by call (and to the closed
form and the leftover flag at an integer-valued step), values bit-equal in exact mode and otherwise inside the rel-RMS
gate AND the per-sample bound of the kernel family (derived in stream_checks' docstring).  Every test prints the worst
per-sample ratio to its bound.  `-m gpu`."""
import functools

import numpy as np
import pytest

import stream_checks as sc
from simplefe_amd import synth

pytestmark = pytest.mark.gpu
B = 4096


@pytest.fixture(scope="module")
def api():
    from simplefe_amd import api as a
    return a


@pytest.fixture(scope="module")
def L():
    from simplefe_amd import lib
    return lib


def _stream(n, cplx, c, seed):
    """channel c of a test stream: n samples, interleaved I/Q when complex"""
    return synth.synth_f32(n * (2 if cplx else 1), ch=seed * 8 + c)


# ------------------------------------------------------------------------------------------------ FIR
FIR_TAPS = {256: synth.taps_cfg2(), 3841: synth.lowpass_taps(3841, 0.1)}


@functools.lru_cache(maxsize=None)
def _fir_ref(n_taps, n, cplx, c, u8=False):
    """(float64 direct convolution, the same on absolute values, the stream as the kernel reads it, the bytes) per float"""
    taps = FIR_TAPS[n_taps].astype(np.float64)
    w = 2 if cplx else 1
    if u8:
        b = np.random.default_rng(100 + c).integers(0, 256, size=w * n, dtype=np.uint8)
        x = ((b.astype(np.float64) - 128.0) * np.float64(np.float32(1.0 / 127.0))).astype(np.float32)
    else:
        b, x = None, _stream(n, cplx, c, 1)
    ref, A = np.empty(w * n), np.empty(w * n)
    for part in range(w):
        xp = x[part::w].astype(np.float64)
        ref[part::w] = np.convolve(xp, taps)[:n]
        A[part::w] = np.convolve(np.abs(xp), np.abs(taps))[:n]
    return ref, A, x, b


def _fir_bound(algo_fft, n_taps, n, cplx, x, A):
    if not algo_fft:
        return sc.direct_bound(A, n_taps)
    # a partitioned filter adds its partitions' transforms: the same form over the window all of them read
    return sc.transform_bound(x, FIR_TAPS[n_taps], 4096, 4096 + n_taps, np.arange(n), cplx=cplx)


def _fir_case(api, L, n_taps, n, algo, cplx, nch, cuts=None, aligned=True):
    f = api.Fir(FIR_TAPS[n_taps], data_complex=cplx, n_channels=nch, algo=algo)
    refs = [_fir_ref(n_taps, n, cplx, c) for c in range(nch)]
    x = np.stack([r[2] for r in refs])
    y = sc.run_fir(api, f, x, cuts=cuts, aligned=aligned)
    worst = 0.0
    for c in range(nch):
        bound = _fir_bound(algo == L.FIR_ALGO_FFT, n_taps, n, cplx, refs[c][2], refs[c][1])
        # rel-RMS 1e-5 everywhere, but for the transform kernel on a call shorter than the filter: such a call holds only the
        # start of the low-pass's transient (|y| ~ 1e-4 of full scale for n = 1, taps_cfg2's edge taps), while the transform's
        # error is relative to the whole block's norm (~1e-7 of it), so there the figure has no derivation and only the
        # per-sample bound, which is absolute, applies
        tol = np.inf if algo == L.FIR_ALGO_FFT and n < n_taps else 1e-5
        worst = max(worst, sc.check_values(y[c], refs[c][0].astype(np.float32), bound=bound, tol=tol, label="channel %d" % c))
    f.close()
    print("FIR %d taps n %d %s %s x%d: worst per-sample ratio %.4f" % (n_taps, n, "FFT" if algo == L.FIR_ALGO_FFT else "DIRECT",
                                                                       "cf32" if cplx else "f32", nch, worst))


@pytest.mark.parametrize("nch", [1, 3])
@pytest.mark.parametrize("cplx", [True, False])
@pytest.mark.parametrize("algo", ["DIRECT", "FFT"])
@pytest.mark.parametrize("n", [1, 255, 3840, 3841, 8193])
def test_fir_256_taps_around_the_tile(api, L, n, algo, cplx, nch):
    """one tile, the tile's advance (3840 for 256 taps) and one more, two tiles and one more; in one call"""
    _fir_case(api, L, 256, n, getattr(L, "FIR_ALGO_" + algo), cplx, nch)


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("cplx", [True, False])
@pytest.mark.parametrize("algo", ["DIRECT", "FFT"])
def test_fir_256_taps_cut_with_carried_state(api, L, algo, cplx, aligned):
    """calls of 1, B - 1 and the rest: the history of a one-sample call, of a call shorter than a tile and of a long one;
    and the same from channels that start one sample off a 16-byte boundary at an odd stride"""
    _fir_case(api, L, 256, 8193, getattr(L, "FIR_ALGO_" + algo), cplx, 3, cuts=[0, 1, B, 8193], aligned=aligned)


@pytest.mark.parametrize("nch", [1, 3])
@pytest.mark.parametrize("cplx", [True, False])
def test_fir_3841_taps_partitioned(api, L, cplx, nch):
    plan = api._l.load()
    import ctypes as C
    ovl, parts, adv = C.c_int(0), C.c_int(0), C.c_int(0)
    api.check(plan.sfe_dsp_fir_plan(3841, C.byref(ovl), C.byref(parts), C.byref(adv)))
    assert parts.value > 1
    _fir_case(api, L, 3841, 9000, L.FIR_ALGO_FFT, cplx, nch)
    _fir_case(api, L, 3841, 9000, L.FIR_ALGO_FFT, cplx, nch, cuts=[0, 1, B, 9000])


def test_fir_u8_input(api, L):
    n, nch = 8193, 3
    f = api.Fir(FIR_TAPS[256], data_complex=True, n_channels=nch, algo=L.FIR_ALGO_FFT)
    f.set_input_format(L.FMT_U8)
    refs = [_fir_ref(256, n, True, c, True) for c in range(nch)]
    y = sc.run_fir(api, f, np.stack([r[3] for r in refs]), cuts=[0, 3841, n], in_u8=True)
    worst = max(sc.check_values(y[c], refs[c][0].astype(np.float32),
                                bound=_fir_bound(True, 256, n, True, refs[c][2], None)) for c in range(nch))
    print("FIR u8 input: worst per-sample ratio %.4f" % worst)


@pytest.mark.parametrize("cplx", [True, False])
def test_fir_tx10_output(api, L, orc, cplx):
    """the packed groups, guarded byte for byte, equal the converter applied to the float output of the same calls"""
    n, nch = 8193, 3                                   # one trailing sample forms no group
    per_group = 2 if cplx else 4
    x = np.stack([0.6 * _fir_ref(256, n, cplx, c)[2] for c in range(nch)]).astype(np.float32)
    f = api.Fir(FIR_TAPS[256], data_complex=cplx, n_channels=nch, algo=L.FIR_ALGO_FFT)
    yf = sc.run_fir(api, f, x)
    g = api.Fir(FIR_TAPS[256], data_complex=cplx, n_channels=nch, algo=L.FIR_ALGO_FFT)
    g.set_output_format(L.FMT_TX10)
    yb = sc.run_fir(api, g, x, out_tx10=True)
    groups, worst = n // per_group, 0.0
    assert yb.shape == (nch, 5 * groups)
    for c in range(nch):
        assert np.array_equal(yb[c], orc.tx_f32_to_10bit(yf[c][: 4 * groups])), c
        ref = 0.6 * _fir_ref(256, n, cplx, c)[0]
        worst = max(worst, sc.check_values(yf[c], ref.astype(np.float32), bound=0.6 * _fir_bound(True, 256, n, cplx, _fir_ref(256, n, cplx, c)[2], None)))
    print("FIR TX10 output %s: worst per-sample ratio %.4f" % ("cf32" if cplx else "f32", worst))


# ------------------------------------------------------------------------------------------------ integer-valued steps
# name: (taps, U, S, n)
INT_SHAPES = {
    "5/3 x 381 n 8000": (synth.taps_cfg3(), 3, 5, 8000),
    "5/3 x 381 n 2000": (synth.taps_cfg3(), 3, 5, 2000),
    "5/3 x 381 n 2002": (synth.taps_cfg3(), 3, 5, 2002),
    "/8 x 64": (synth.taps_cfg4(), 1, 8, 8001),
    "x3": (synth.lowpass_taps(95, 0.15, gain=3.0), 3, 1, 3000),
    "/63": (synth.lowpass_taps(505, 0.9 / 63.0), 1, 63, 9014),
    "10/9": (synth.lowpass_taps(271, 0.045, gain=9.0), 9, 10, 5000),
}
_pending = {k: sc.closed_form_total(n, U, S) * S - n * U == -1 for k, (_, U, S, n) in INT_SHAPES.items()}
assert any(_pending.values()) and not all(_pending.values()), _pending          # streams that end on a pending leftover, and not


def _cuts3(n, blk):
    return sorted({0, 1, min(blk, n), n})


@functools.lru_cache(maxsize=None)
def _rs_ref(orc, key, rate, blk, cuts, cplx, c, mode="resample"):
    """the float32 oracle over one channel (per component), the same on absolute values, its per-call counts"""
    taps, U = key
    taps = np.frombuffer(taps, np.float32)
    n = cuts[-1]
    w = 2 if cplx else 1
    x = _stream(n, cplx, c, 2)
    cls = orc.Resample if mode == "resample" else orc.Decimate
    parts, absp, counts = [], [], None
    for part in range(w):
        xp = np.ascontiguousarray(x[part::w])
        y, ks = sc.reference_stream(cls(taps, U, blk), xp, rate, list(cuts), blk)
        a, _ = sc.reference_stream(cls(np.abs(taps), U, blk), np.abs(xp), rate, list(cuts), blk)
        parts.append(y)
        absp.append(a)
        assert counts is None or counts == ks
        counts = ks
    ref, A = np.empty(w * len(parts[0]), np.float32), np.empty(w * len(parts[0]), np.float32)
    for part in range(w):
        ref[part::w], A[part::w] = parts[part], absp[part]
    return ref, A, counts, x


@functools.lru_cache(maxsize=None)
def _law_end(n, U, rate, cuts, blk):
    return sc.law_positions(n, U, rate, list(cuts), blk)[3]


def _rs_case(api, L, orc, taps, U, rate, blk, cuts, cplx, nch, exact, algo, bound_of, S=None, mode="resample", aligned=True, label=""):
    n = cuts[-1]
    r = api.Rs(taps, U, blk, mode=L.RS_RESAMPLE if mode == "resample" else L.RS_DECIMATE, data_complex=cplx, n_channels=nch)
    r.set_exact(exact)
    if algo is not None:
        r.set_algo(algo)
    refs = [_rs_ref(orc, (taps.tobytes(), U), rate, blk, tuple(cuts), cplx, c, mode) for c in range(nch)]
    x = np.stack([q[3] for q in refs])
    y, counts = sc.run_rs(api, r, x, rate, cuts=cuts, aligned=aligned)
    sc.check_counts(counts, refs[0][2], r.get_state(), n, U, S)
    worst = 0.0
    for c in range(nch):
        ref, A = refs[c][0], refs[c][1]
        if exact:
            sc.check_values(y[c], ref, exact=True, label="channel %d" % c)
        else:
            worst = max(worst, sc.check_values(y[c], ref, bound=bound_of(refs[c][3], A, counts), label="channel %d" % c))
    pending = bool(r.get_state().leftover)
    if S is None:
        assert pending == _law_end(n, U, rate, tuple(cuts), blk)
    r.close()
    print("%s %s %s x%d: counts %s, leftover pending %s, worst per-sample ratio %.4f"
          % (label, "exact" if exact else "fused", "cf32" if cplx else "f32", nch, counts, pending, worst))
    return pending


def _int_bound(taps, U, S, cuts, cplx, algo_direct):
    """direct sums, except the outputs of a call that the transform-domain kernel may take (fused, K >= 4096,
    include/sfe_dsp.h): those are held to whichever of the two bounds is wider"""
    Lp = -(-len(taps) // U)
    SP = S // int(np.gcd(U, S))
    w = 2 if cplx else 1

    def bound_of(x, A, counts):
        b = sc.direct_bound(A, Lp)
        k0 = 0
        for k in counts:
            if k >= 4096 and not algo_direct:
                pos = (np.arange(k0, k0 + k) * S) // U
                tb = sc.transform_bound(x, taps, 256, 256 * SP + Lp, pos, U=U, cplx=cplx)
                b[w * k0:w * (k0 + k)] = np.maximum(b[w * k0:w * (k0 + k)], tb)
            k0 += k
        return b
    return bound_of


@pytest.mark.parametrize("nch", [1, 3])
@pytest.mark.parametrize("cplx", [True, False])
@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("name", list(INT_SHAPES))
def test_integer_step_cut_at_one_sample_and_one_block(api, L, orc, name, exact, cplx, nch):
    taps, U, S, n = INT_SHAPES[name]
    rate = float(np.float32(S) / np.float32(U))
    cuts = _cuts3(n, B)
    pending = _rs_case(api, L, orc, taps, U, rate, B, cuts, cplx, nch, exact, None, _int_bound(taps, U, S, cuts, cplx, False), S=S, label=name)
    assert pending == _pending[name]


@pytest.mark.parametrize("nch", [1, 3])
@pytest.mark.parametrize("cplx", [True, False])
@pytest.mark.parametrize("algo", ["AUTO", "FFT", "DIRECT"])
def test_integer_step_5_3_in_one_call_reaches_the_transform_kernel(api, L, orc, algo, cplx, nch):
    """n = 8000 in ONE call: K = 4800 just reaches the transform-domain kernel's K >= 4096"""
    taps, U, S, n = INT_SHAPES["5/3 x 381 n 8000"]
    assert sc.closed_form_total(n, U, S) == 4800
    _rs_case(api, L, orc, taps, U, float(np.float32(5) / np.float32(3)), B, [0, n], cplx, nch, False, getattr(L, "RS_ALGO_" + algo),
             _int_bound(taps, U, S, [0, n], cplx, algo == "DIRECT"), S=S, label="5/3 x 381 one call " + algo)


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("name", ["/8 x 64", "/63", "5/3 x 381 n 2002"])
def test_integer_step_decimate_mode_and_unaligned_channels(api, L, orc, name, exact):
    """SFE_RS_DECIMATE (the decimate class: the same law, libdsp/test/test_decimate.py:36) from channels one sample off a
    16-byte boundary at an odd stride: the kernels the LDS-DMA forms replace"""
    taps, U, S, n = INT_SHAPES[name]
    cuts = _cuts3(n, B)
    _rs_case(api, L, orc, taps, U, float(np.float32(S) / np.float32(U)), B, cuts, False, 3, exact, None,
             _int_bound(taps, U, S, cuts, False, False), S=S, mode="decimate", aligned=False, label=name + " decimate, unaligned")


# ------------------------------------------------------------------------------------------------ the general rate
GEN_TAPS, GEN_U = synth.taps_cfg3(), 3
# (rate, blksize, cuts) of the streams below
GEN_STREAMS = [(rate, blk, [0, 3 * blk, 5 * blk + blk // 3]) for rate in (1.77, 0.77) for blk in (256, 4096)] + \
              [(rate, B, [0, 1, B, 5 * B + B // 3 + 2]) for rate in (1.77, 0.77)]


def _gen_bound(blk, n, rate, cplx, kind):
    Lp = 127
    w = 2 if cplx else 1

    def bound_of(x, A, counts):
        d = sc.direct_bound(A, Lp)
        if kind != "FFT":
            return d
        pos = np.minimum((np.arange(len(A) // w) * np.float64(rate)).astype(np.int64), n - 1)
        t = sc.transform_bound(x, GEN_TAPS, 4096, (4096 if cplx else 8192) + Lp, pos, U=GEN_U, cplx=cplx)
        # blksize 4096: poly_gen.hip.  A small blksize leaves the direct kernel in charge (include/sfe_dsp.h): whichever ran,
        # it is inside the wider of the two
        return t if blk >= 4096 else np.maximum(t, d)
    return bound_of


@pytest.mark.parametrize("nch", [1, 3])
@pytest.mark.parametrize("cplx", [True, False])
@pytest.mark.parametrize("kind", ["exact", "DIRECT", "FFT"])
@pytest.mark.parametrize("blk", [256, 4096])
@pytest.mark.parametrize("rate", [1.77, 0.77])
def test_general_rate_in_calls_of_three_blocks(api, L, orc, rate, blk, kind, cplx, nch):
    """n = 5 B + B/3 in calls of 3 B: a whole number of reference calls, then a ragged last one"""
    rate = float(np.float32(rate))
    n = 5 * blk + blk // 3
    cuts = [0, 3 * blk, n]
    _rs_case(api, L, orc, GEN_TAPS, GEN_U, rate, blk, cuts, cplx, nch, kind == "exact", None if kind == "exact" else getattr(L, "RS_ALGO_" + kind),
             _gen_bound(blk, n, rate, cplx, kind), label="rate %.2f blksize %d %s" % (rate, blk, kind))


@pytest.mark.parametrize("kind", ["exact", "FFT"])
@pytest.mark.parametrize("rate", [1.77, 0.77])
def test_general_rate_cut_inside_a_reference_call(api, L, orc, rate, kind):
    """calls of 1, B - 1 and the rest at a non-integer step: the GPU's law replays blksize-sample calls from each bulk call's
    start, and the oracle is fed those boundaries"""
    rate = float(np.float32(rate))
    n = 5 * B + B // 3 + 2
    cuts = [0, 1, B, n]
    _rs_case(api, L, orc, GEN_TAPS, GEN_U, rate, B, cuts, True, 3, kind == "exact", None if kind == "exact" else L.RS_ALGO_FFT,
             _gen_bound(B, n, rate, True, kind), label="rate %.2f cut at 1 and B, %s" % (rate, kind))
