"""The three streaming measurement blocks (csrc/psd.hip, corr.hip, iir.hip) through the poisoned, guarded, strided buffers of
tests/stream_checks.py (run_psd, run_corr, run_iir): every input stream at an offset inside a buffer of NaN with
in_stride > n_in, every output poisoned before every call between a front guard, gaps and a tail guard with its stride
greater than its payload, every buffer read back whole after every call, counts held to their closed forms.  `-m gpu`.
tests/test_measure_checks_host.py shows on the CPU that the runners catch what they are here to catch.

No bar is new: PSD and the correlator are held to the project's TOL = 1e-5 as in test_gpu_psd.py and test_gpu_corr.py, the
IIR to the multiples (4; 12 with a DC offset) of the float32 yardstick of test_gpu_iir.py, whose _check and _yard are used
as they are.  What is new is the shapes: every PSD size (N = 512 and 2048 take the radix-2 first pass, N = 512 alone has two
segments to a batch), the IIR's three formats with three streams across a group of the fold, the correlator's overlap rows
3 to 7 and every path of its energy-window walk.  Every case prints its worst error beside its bar.

The PSD grid is the product N x H x A x streams trimmed to 25 cases so that every N meets every H, every A and both stream
counts: with i the index of H in (N, N/2, 3N/8 + 1, N - 1) and j the index of N, A = (1, 2, 3, 5)[(i + j) % 4] and
streams = (1, 3)[(i + j) % 2]; H = 1 (a call far shorter than one segment, N - 1 samples of history) runs with 3 streams at
A = 1 for N = 256, 1024, 4096 and A = 5 for N = 512, 2048.  PSD_GRID below is that list."""
import numpy as np
import pytest

import stream_checks as sc
import test_gpu_corr as tc
import test_gpu_iir as ti
from simplefe_amd import synth

pytestmark = pytest.mark.gpu
TOL = 1e-5
SIZES = (256, 512, 1024, 2048, 4096)


@pytest.fixture(scope="module")
def api():
    from simplefe_amd import api as a
    return a


@pytest.fixture(scope="module")
def L():
    from simplefe_amd import lib
    return lib


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ================================================================================================ PSD
def _hops(N):
    return {"N": N, "N/2": N // 2, "3N/8+1": 3 * N // 8 + 1, "N-1": N - 1, "1": 1}


PSD_GRID = []
for _j, _N in enumerate(SIZES):
    for _i, _h in enumerate(("N", "N/2", "3N/8+1", "N-1")):
        PSD_GRID.append((_N, _h, (1, 2, 3, 5)[(_i + _j) % 4], (1, 3)[(_i + _j) % 2]))
    PSD_GRID.append((_N, "1", (1, 5)[_j % 2], 3))
assert len(PSD_GRID) == 25
for _N in SIZES:        # every N with every H, every A and both stream counts
    assert {g[1] for g in PSD_GRID if g[0] == _N} == {"N", "N/2", "3N/8+1", "N-1", "1"}
    assert {g[2] for g in PSD_GRID if g[0] == _N} == {1, 2, 3, 5} and {g[3] for g in PSD_GRID if g[0] == _N} == {1, 3}


def _psd_streams(n, n_streams, first=0):
    return np.stack([synth.synth_cf32(n, ch=s, first_sample=first).view(np.complex64) for s in range(n_streams)])


def _psd_errors(got, ref):
    """(rel-RMS over the bins, worst bin error over the row's RMS) of one row, as test_gpu_psd.py takes them."""
    err = got.astype(np.float64) - ref
    rms = np.sqrt(np.mean(ref ** 2))
    return np.sqrt(np.mean(err ** 2)) / rms, np.abs(err).max() / rms


def _psd_held(tag, y, x, w, H, A, scale):
    """Every row of every stream against synth.psd_reference; returns the worst (rel-RMS, bin)."""
    wr = ww = 0.0
    for s in range(y.shape[0]):
        ref = synth.psd_reference(x[s], w, H, A, np.float32(scale))
        assert ref.shape == y[s].shape, (tag, ref.shape, y.shape)
        for r in range(ref.shape[0]):
            if not ref[r].any():
                # H = 1, segment 0: N - 1 zeros and x[0] under the Hann window's last value, which is 0.  Nothing to be
                # relative to: the row must be zero itself
                assert not y[s, r].any(), (tag, s, r, "a row of zeros in the reference")
                continue
            rel, worst = _psd_errors(y[s, r], ref[r])
            assert rel <= TOL and worst <= TOL, (tag, s, r, rel, worst)
            wr, ww = max(wr, rel), max(ww, worst)
    print("psd %s: worst rel-RMS %.2e worst bin %.2e (bar %.0e)" % (tag, wr, ww, TOL))
    return wr, ww


@pytest.mark.timeout(300)
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("N, hop_of, A, n_streams", PSD_GRID)
def test_psd_parity_grid(api, N, hop_of, A, n_streams, aligned):
    H = _hops(N)[hop_of]
    w = np.hanning(N).astype(np.float32)
    scale = 1.0 / (A * float(np.sum(w.astype(np.float64) ** 2)))
    n = (2 * A + 3) * H                     # two rows complete, a third stays open (A = 1: five rows)
    x = _psd_streams(n, n_streams)
    ps = api.Psd(w, H, A, scale=scale, n_streams=n_streams)
    y, counts = sc.run_psd(api, ps, x, aligned=aligned)
    ps.close()
    assert counts == [(2 * A + 3) // A]
    tag = "grid N=%d H=%d A=%d S=%d %s" % (N, H, A, n_streams, "aligned" if aligned else "unaligned")
    _psd_held(tag, y, x, w, H, A, scale)
    if hop_of == "3N/8+1" and aligned:
        # sixteen spread bins of the last row of the last stream by the written-out DFT sum: no framing code shared
        s, r = n_streams - 1, y.shape[1] - 1
        bins = (np.arange(16) * (N // 16) + 5 * np.arange(16) + 1) % N
        direct = synth.psd_reference_direct(x[s], w, H, A, np.float32(scale), 0, r, bins)
        rms = np.sqrt(np.mean(synth.psd_reference(x[s], w, H, A, np.float32(scale))[r] ** 2))
        worst = np.abs(y[s, r, bins].astype(np.float64) - direct).max() / rms
        print("psd %s: 16 bins of row %d against the direct sum, worst %.2e (bar %.0e)" % (tag, r, worst, TOL))
        assert worst <= TOL, (tag, worst)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("A", [2, 5])
@pytest.mark.parametrize("H", [97, 201])
@pytest.mark.parametrize("N", [256, 512])
def test_psd_batch_tails(api, N, H, A):
    """N = 256 transforms four segments at a time, N = 512 two.  Calls of 1, 2, 3, 5 and 7 segments, twice over: the pieces
    hold every residue of segments modulo 4 and 2, and start in mid-chunk and on chunk edges (A = 2: C = 2, a chunk is a
    row; A = 5: C = 4, chunks of 4 and 1).  The bits are the one call's, and the one call is held to the reference."""
    S, calls = 3, [1, 2, 3, 5, 7] * 2
    segs = sum(calls)
    w = np.hanning(N).astype(np.float32)
    x = _psd_streams(segs * H, S)
    one, k = sc.run_psd(api, api.Psd(w, H, A, scale=0.37, n_streams=S), x)
    assert k == [segs // A]
    _psd_held("batch tails N=%d H=%d A=%d, one call" % (N, H, A), one, x, w, H, A, 0.37)
    cuts = [0] + [int(c) * H for c in np.cumsum(calls)]
    got, counts = sc.run_psd(api, api.Psd(w, H, A, scale=0.37, n_streams=S), x, cuts)
    before = np.concatenate([[0], np.cumsum(calls)[:-1]])
    assert counts == [int((b % A + c) // A) for b, c in zip(before, calls)]
    C, rows_per_batch = api.psd_plan(N, H, A)[0], 1024 // N
    assert {int(b % C == 0) for b in before % A} == {0, 1}         # pieces start on chunk edges and inside chunks
    # a piece is the part of one chunk inside one call: with chunks of 4 (A = 5) their lengths take every residue modulo
    # the batch, with chunks of 2 (A = 2) the residues 1 and 2
    pieces = {}
    for i, (b, c) in enumerate(zip(before, calls)):
        for m in range(int(b), int(b) + c):
            key = (i, m // A, (m % A) // C)
            pieces[key] = pieces.get(key, 0) + 1
    assert {v % rows_per_batch for v in pieces.values()} == {v % rows_per_batch for v in range(1, C + 1)}
    assert got.shape == one.shape and np.array_equal(_bits(got), _bits(one)), (N, H, A)


def _cut(total, step):
    return [step] * (total // step) + ([total % step] if total % step else [])


@pytest.mark.timeout(300)
@pytest.mark.parametrize("N, H, A, irregular", [
    # C = 8, a row's chunks hold 8, 8, 8, 8, 5 segments: cuts inside a chunk, on a chunk edge, inside a row, on a row edge
    (512, 201, 37, [3, 5, 20, 9, 45, 1, 60]),
    # C = 4, chunks of 4 and 1
    (2048, 2048, 5, [2, 2, 1, 3, 13, 1]),
])
def test_psd_cutting_the_stream_gives_the_same_bits(api, N, H, A, irregular):
    """test_gpu_psd.py's cut test at the two sizes it lacks, with three streams and through the guarded buffers.  The calls of
    one segment complete no row but every A-th: those calls must report 0 and leave their whole output buffer poison."""
    S = 3
    assert api.psd_plan(N, H, A)[0] == {37: 8, 5: 4}[A]
    segs = 4 * A + 11
    w = np.hanning(N).astype(np.float32)
    x = _psd_streams(segs * H, S)
    one, k = sc.run_psd(api, api.Psd(w, H, A, scale=0.37, n_streams=S), x)
    assert k == [segs // A] and one.shape == (S, segs // A, N)
    _psd_held("cuts N=%d H=%d A=%d, one call" % (N, H, A), one, x, w, H, A, 0.37)
    irregular = irregular + [segs - sum(irregular)]
    assert irregular[-1] > 0
    for calls in (_cut(segs, 1), _cut(segs, 3), _cut(segs, 7), irregular):
        cuts = [0] + [int(c) * H for c in np.cumsum(calls)]
        got, counts = sc.run_psd(api, api.Psd(w, H, A, scale=0.37, n_streams=S), x, cuts)
        assert sum(counts) == segs // A
        if calls[0] == 1:
            assert counts.count(0) == segs - segs // A
        assert np.array_equal(_bits(got), _bits(one)), (N, H, A, calls[:8])


@pytest.mark.timeout(300)
@pytest.mark.parametrize("N, H, A", [(512, 201, 3), (2048, 1024, 4)])
def test_psd_u8_input_equals_converted_cf32(api, L, N, H, A):
    """Three streams of bytes 2 bytes past a 16-byte boundary at an odd stride, in two calls, against the cf32 path on
    synth.u8_to_cf32 of the same bytes in one."""
    S = 3
    n = (3 * A + 2) * H
    w = np.hanning(N).astype(np.float32)
    b = np.stack([synth.offset_bytes(n, seed=N + s) for s in range(S)])
    xf = np.stack([synth.u8_to_cf32(r) for r in b])
    want, k = sc.run_psd(api, api.Psd(w, H, A, n_streams=S), xf)
    assert k == [3]
    _psd_held("u8 N=%d H=%d A=%d, cf32 of the converted bytes" % (N, H, A), want, xf, w, H, A, 1.0)
    ps = api.Psd(w, H, A, n_streams=S)
    ps.set_input_format(L.FMT_U8)
    got, k = sc.run_psd(api, ps, b, [0, (A + 1) * H, n], in_u8=True, aligned=False)
    assert k == [1, 2]
    assert np.array_equal(_bits(got), _bits(want)), (N, H, A)


# ================================================================================================ IIR
IIR_FILTERS = ["dc(0.9999)", ti.CASCADE, "butter(16,0.1)"]          # S = 1, 5, 8 sections
IIR_FORMATS = ["cf32", "u8", "real"]
IIR_K = 128                                                          # blocks to a group of the fold (csrc/iir.hip)


def _iir_input(fmt, n, S=3):
    """(what the handle is fed, the samples it stands for): the generator fill_synth runs on the device, here on the host."""
    if fmt == "u8":
        b = np.stack([synth.offset_bytes(n, seed=40 + s) for s in range(S)])
        return b, np.stack([synth.u8_to_cf32(r) for r in b])
    if fmt == "real":
        x = np.stack([synth.synth_f32(n, ch=3 + s) for s in range(S)])
        return x, x
    x = np.stack([synth.synth_cf32(n, ch=3 + s).view(np.complex64) for s in range(S)])
    return x, x


def _iir_handle(api, L, fmt, sos, n_streams):
    f = api.Iir(sos, data_complex=fmt != "real", n_streams=n_streams)
    if fmt == "u8":
        f.set_input_format(L.FMT_U8)
    return f


def _iir_lead(sos):
    """Samples before the checked window from which its reference starts at zero state: 16 384, as
    test_cuts_across_the_groups_of_the_fold takes them, where the filter has forgotten its past by then, else the first
    multiple of 16 384 at which the largest pole radius r has r^lead <= 1e-9, three orders below the smallest bar.  At
    r = 0.9999 (dc(0.9999)) r^16384 is 0.19 -- a reference started there would be wrong by a tenth of the output's RMS --
    and the lead is 212 992 samples."""
    r = max(np.abs(np.roots([1.0, a1, a2])).max() for _, _, _, a1, a2 in synth.iir_round(sos).astype(np.float64))
    lead = 16384
    while r ** lead > 1e-9:
        lead += 16384
    return lead


_alone = {}


def _iir_alone(api, L, fmt, name, G, fed):
    """Three one-stream handles fed the 130 blocks in ONE call each, plainly (in_stride == n): the path
    test_cuts_across_the_groups_of_the_fold validates.  Computed once per (format, filter) and left unchanged."""
    if (fmt, name) not in _alone:
        _alone[fmt, name] = np.stack([_iir_handle(api, L, fmt, ti.FILTERS[name], 1).filter(
            row.reshape(-1, 2) if fmt == "u8" else row) for row in fed])
        _alone[fmt, name].setflags(write=False)
    return _alone[fmt, name]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("name", IIR_FILTERS)
@pytest.mark.parametrize("fmt", IIR_FORMATS)
def test_iir_three_streams_across_a_group_of_the_fold(api, L, fmt, name, aligned):
    """130 blocks of three streams: 126 in the handle's first call, then calls of 1, 2 and 1 blocks -- the last block of a
    group, a call that straddles the group boundary, the first block of the new group -- with NC = 2 (cf32, u8) and NC = 1
    (real) in the state tables' indices.  in_stride != out_stride, both greater than n, both odd multiples of 16 bytes
    (aligned) or odd counts of samples (unaligned: cf32 8, u8 2, real 4 bytes past a 16-byte boundary)."""
    G = api.iir_plan(synth.iir_one_pole(0.5))[0]
    sos, nb = ti.FILTERS[name], IIR_K + 2
    n = nb * G
    fed, x = _iir_input(fmt, n)
    item, osz = {"cf32": 8, "u8": 2, "real": 4}[fmt], 4 if fmt == "real" else 8
    for m in (G, 2 * G, 126 * G):
        si, so = sc.measure_strides(m, item, m, osz, aligned)
        assert si > m and so > m and si != so and si % 2 == so % 2 == (0 if aligned else 1)
    f = _iir_handle(api, L, fmt, sos, 3)
    y = sc.run_iir(api, f, fed, [0, (IIR_K - 2) * G, (IIR_K - 1) * G, (IIR_K + 1) * G, n], in_u8=fmt == "u8", aligned=aligned)
    f.close()
    alone = _iir_alone(api, L, fmt, name, G, fed)
    assert y.shape == alone.shape == x.shape and y.dtype == alone.dtype
    for s in range(3):
        assert np.array_equal(_bits(y[s]), _bits(alone[s])), (fmt, name, s, "the bits of a one-stream handle's one call")
    at, lead = n - 4096, _iir_lead(sos)
    ref, y32 = ti._yard(("guarded window", fmt, name), x[:, at - lead:], sos)
    for s in range(3):
        ti._check("guarded %s %s %s, s=%d, last window of 130 blocks" % (fmt, name, "aligned" if aligned else "unaligned", s),
                  y[s, at:], ref[s, lead:], y32[s, lead:], 4)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("fmt", IIR_FORMATS)
def test_iir_three_blocks_of_three_streams(api, L, fmt, aligned):
    """in_stride = n + 7 and out_stride = n + 5 items, the whole float64 reference for every stream, a filter whose ringing
    crosses the block edges: stream s depends visibly on its own state, and on no other's."""
    name = "dc(0.9999)"
    G = api.iir_plan(synth.iir_one_pole(0.5))[0]
    n = 3 * G
    fed, x = _iir_input(fmt, n)
    f = _iir_handle(api, L, fmt, ti.FILTERS[name], 3)
    y = sc.run_iir(api, f, fed, [0, n], in_u8=fmt == "u8", aligned=aligned, strides=lambda n_in, n_out: (n_in + 7, n_out + 5))
    f.close()
    ref, y32 = ti._yard(("guarded three blocks", fmt), x, ti.FILTERS[name])
    for s in range(3):
        ti._check("guarded three blocks %s %s, s=%d" % (fmt, "aligned" if aligned else "unaligned", s), y[s], ref[s], y32[s], 4)


# ================================================================================================ correlator
def _corr_held(tag, ref_m, B, val, idx, m):
    """One stream against its float64 reference (K, n): the dense values where there are any, every block's peak value, and
    that the reported offset attains the block's maximum (to 2 TOL, as test_gpu_corr.py holds it).  peak_idx is uint32."""
    K, n = ref_m.shape
    assert idx.dtype == np.uint32 and val.shape == idx.shape == (K, n // B)
    assert (idx < B).all(), (tag, "an offset outside its block")
    wm = float(np.abs(m.astype(np.float64) - ref_m).max()) if m is not None else 0.0
    assert wm <= TOL, (tag, "dense", wm)
    blocks = ref_m.reshape(K, n // B, B)
    top = blocks.max(axis=2)
    wp = float(np.abs(val.astype(np.float64) - top).max())
    assert wp <= TOL, (tag, "peak", wp)
    at = np.take_along_axis(blocks, idx.astype(np.int64)[:, :, None], axis=2)[:, :, 0]
    assert (at >= top - 2 * TOL).all(), (tag, "the reported offset does not attain the maximum")
    return wm, wp


# L, the thread rows of overlap m0 = (4096 - V) / 256, the path of the energy-window walk.  On the float64 reference alone
# the planted peak exceeds every other value of its block by 0.05 at every one of these lengths with test_gpu_corr.py's
# NOISE_SEED, computed on the CPU before any GPU run: margins 0.41 (L = 33), 0.094 (300), 0.13 (600), 0.10 (1100), 0.087
# (1793), 0.090 (1794) at the shapes below, and 0.15 / 0.34 / 0.10 / 0.11 at L = 13 / 257 / 1100 / 2049 with four blocks
# (test_corr_gaps_everywhere).  No case needed a seed of its own.
CORR_LENGTHS = [(33, 1), (300, 2), (600, 3), (1100, 5), (1793, 7), (1794, 8)]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("ratio", [1, 2], ids=["B=V", "B=2V"])
@pytest.mark.parametrize("Lt, m0", CORR_LENGTHS)
def test_corr_overlap_rows_and_the_energy_walk(api, Lt, m0, ratio):
    V = tc._advance(Lt)
    assert (4096 - V) // 256 == m0 and api.corr_plan(Lt, 2, ratio * V) == (V, 4096 - V)
    B = ratio * V
    n, S, K = 3 * B, 2, 2
    x = np.stack([tc._case(Lt, n, s)[0] for s in range(S)])
    cr = api.Corr(tc._templates(Lt)[:K], B, tc.GATE, n_streams=S)
    val, idx, m, counts = sc.run_corr(api, cr, x)
    cr.close()
    assert counts == [3]
    wm, wp = tc._check_parity(Lt, K, B, x, val, idx, m, (Lt, ratio))
    print("corr guarded L=%d m0=%d B=%dV S=%d K=%d: worst dense %.2e worst peak %.2e (bar %.0e)" % (Lt, m0, ratio, S, K, wm, wp, TOL))


@pytest.mark.timeout(300)
@pytest.mark.parametrize("dense", [True, False], ids=["dense", "peaks"])
@pytest.mark.parametrize("fmt", ["cf32", "u8"])
@pytest.mark.parametrize("Lt, ratio", [(13, 1), (257, 2), (1100, 1), (2049, 2)])
def test_corr_gaps_everywhere(api, L, Lt, ratio, fmt, dense):
    """Three streams, three templates, calls of B, 2B and B with every buffer strided and guarded: the bits of the three
    calls are the one call's, and the one call is held to the reference (of the converted bytes for u8; those are the
    noise-and-templates stream quantised, so that there is something to find)."""
    B = ratio * tc._advance(Lt)
    n, S, K = 4 * B, 3, 3
    t = tc._templates(Lt)[:K]
    x = np.stack([tc._case(Lt, n, s)[0] for s in range(S)])
    u8 = fmt == "u8"
    if u8:
        fed = np.clip(np.round(x.view(np.float32) * np.float32(64.0) + np.float32(128.0)), 0, 255).astype(np.uint8)
        x = np.stack([synth.u8_to_cf32(r) for r in fed])
    else:
        fed = x

    def handle():
        cr = api.Corr(t, B, tc.GATE, n_streams=S)
        if u8:
            cr.set_input_format(L.FMT_U8)
        return cr

    one = sc.run_corr(api, handle(), fed, in_u8=u8, dense=dense, aligned=False)
    assert one[3] == [4] and (one[2] is None) == (not dense)
    wm = wp = 0.0
    for s in range(S):
        ref = tc._case(Lt, n, s)[1][:K] if not u8 else synth.corr_reference(x[s], t, B, tc.GATE)[0]
        a, b = _corr_held((Lt, ratio, fmt, dense, s), ref, B, one[0][s], one[1][s], one[2][s] if dense else None)
        wm, wp = max(wm, a), max(wp, b)
    print("corr gaps L=%d B=%dV %s %s: worst dense %.2e worst peak %.2e (bar %.0e)" % (Lt, ratio, fmt, "dense" if dense else "peaks", wm, wp, TOL))
    if not u8 and dense:
        tc._check_parity(Lt, K, B, x, one[0], one[1], one[2], (Lt, ratio, "gaps"))
    got = sc.run_corr(api, handle(), fed, [0, B, 3 * B, n], in_u8=u8, dense=dense, aligned=True)
    assert got[3] == [1, 2, 1]
    for a, b in zip(got[:3], one[:3]):
        assert (a is None and b is None) or np.array_equal(_bits(a), _bits(b)), (Lt, ratio, fmt, dense)
