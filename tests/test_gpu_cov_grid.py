"""Every class of the covariance estimator's chunk kernel (csrc/cov.hip: cov_chunk_kernel<NT, U8>, NT = 1 .. 8) on the GPU,
held to the summation order of include/sfe_dsp.h BIT FOR BIT.  `-m gpu`.

GRID_S is the lower and the upper edge of every NT = ceil(S / 8): the lower edge has the most zeroed padding rows in its
last tile (2 of 16 rows carry data), the upper edge none.  Between them they reach what tests/test_gpu_cov.py's
S = 1, 2, 3, 8, 9, 33, 64 do not: NT = 3, 4, 6, 7, the classes where a wave owns a phantom tile (NT = 3: six tiles over
four waves) and where the row kernel's blocks of four tiles are partly empty (6, 10 and 21 tiles).

Per S, with M = 2 bands, for A in (T, 2T, 5T) and both input formats, a stream of n = 3A + 2T instants runs once in one
call and, after reset, cut into calls of [1, 2, 1, rest] chunks: with A = T every cut is a row end; with A = 2T (one
group of two chunks) the group is carried into a call that then takes the chunk kernel's direct store; with A = 5T
(groups of 4 and 1) the cuts fall mid-group and mid-row.  The carried sums and the scratch are indexed with the class's
own FR = NTILES 256 floats.  All of it through guarded buffers (test_gpu_cov.Rows): the input rows one element into a
buffer of NaN patterns (u8: 0xFF) with in_stride > n, the output rows inside a sentinel with out_stride > payload.

Asserted: the one-call rows equal synth.cov_law_reference in their bits (u8: on the converted samples); the cut run equals
the one-call run in its bits; every call's row count is floor((instants before mod A + n_in) / A); a call that completes
no row, and every row not yet due, leaves the sentinel; guards, gaps and the input are unchanged; and test_gpu_cov._check
against float64 under its derived bound, unchanged.  No tolerance is new.  Every case prints the floats it compared and
its worst float64 error over the bound."""
import numpy as np
import pytest

import test_gpu_cov as tc
from simplefe_amd import synth

pytestmark = pytest.mark.gpu
T = tc.T
GRID_S = [1, 8, 9, 16, 17, 24, 25, 32, 33, 40, 41, 48, 49, 56, 57, 64]
GRID_A = (T, 2 * T, 5 * T)
CUT_CHUNKS = [1, 2, 1]              # then the rest
M = 2
NMAX = 3 * max(GRID_A) + 2 * T


@pytest.fixture(scope="module")
def api():
    from simplefe_amd import api as a
    assert a.cov_plan(1, 1, T)[0] == T
    return a


@pytest.fixture(scope="module")
def L():
    from simplefe_amd import lib
    return lib


def _run(api, cov, up, cuts, u8):
    """The calls `cuts` (instants each) over one guarded input buffer and into one guarded output buffer of exactly the
    rows the stream completes: (rows (M, rows, 2S, 2S) float32, n_rows of every call).  Asserts on the way what is about
    memory: after every call the guards and gaps of the output and every row not yet due are the sentinel, a call that
    completed no row changed nothing at all, and at the end the input buffer is what was uploaded."""
    S, A, n = cov.n_in, cov.n_avg, sum(cuts)
    gram, most, esz = 4 * S * S, n // A, 2 if u8 else 8
    src = tc.Rows(api, S * M, n, esz, tc.FF_BYTES if u8 else tc.NAN_BYTES, 3, 1).upload(up)
    dst = tc.Rows(api, M, most * gram, 4, tc.SENT_BYTES, 5, 3).upload(np.full((M, most * gram), tc.SENT, np.float32))
    assert src.stride > n and dst.stride > most * gram
    counts, at, done = [], 0, 0
    try:
        image, _ = dst.download()
        for m in cuts:
            k = cov.process_stream(src.ptr + at * esz, m, dst.ptr + done * gram * 4, in_stride=src.stride, out_stride=dst.stride)
            api.sync()
            counts.append(k)
            pay, intact = dst.download()
            assert intact, (cuts, at)
            if k == 0:
                assert np.array_equal(pay, image), (cuts, at)
            at, done, image = at + m, done + k, pay
            assert done <= most and (pay.view(np.uint32)[:, done * gram:] == tc._bits(tc.SENT)).all(), (cuts, at)
        back, in_intact = src.download()
    finally:
        src.free()
        dst.free()
    assert done == most
    assert in_intact and np.array_equal(back, np.ascontiguousarray(up).view(np.uint8).reshape(S * M, n * esz))
    return np.ascontiguousarray(image.view(np.float32).reshape(M, most, 2 * S, 2 * S)), counts


def _row_counts(cuts, A):
    out, before = [], 0
    for m in cuts:
        out.append((before % A + m) // A)
        before += m
    return out


def _differing(got, law):
    """Where two arrays differ in their bits, for the assertion's message: how many, and the first few with both values."""
    g, w = tc._bits(got).ravel(), tc._bits(law).ravel()
    at = np.flatnonzero(g != w)
    return {"floats": int(g.size), "differ": int(at.size),
            "first": [(tuple(int(v) for v in np.unravel_index(i, got.shape)), "%08x" % g[i], "%08x" % w[i]) for i in at[:4]]}


@pytest.mark.parametrize("S", GRID_S)
def test_every_class_gives_the_bits_of_the_law_in_one_call_and_cut(api, L, S):
    for A in GRID_A:
        n, scale = 3 * A + 2 * T, float(np.float32(0.75 / A))           # no power of two: where scale multiplies shows
        chunks = CUT_CHUNKS + [n // T - sum(CUT_CHUNKS)]
        assert chunks[-1] >= 1
        cuts = [c * T for c in chunks]
        cov = api.Cov(S, M, A, scale)
        for u8 in (False, True):
            tag = "S=%d (NT=%d) A=%dT %s" % (S, (2 * S + 15) // 16, A // T, "u8" if u8 else "cf32")
            cov.set_input_format(L.FMT_U8 if u8 else L.FMT_F32)
            up, x = tc._input(S, M, NMAX, u8)
            up, x = np.ascontiguousarray(up[:, :, :(2 if u8 else 1) * n]), np.ascontiguousarray(x[:, :, :n])
            cov.reset()
            one, counts = _run(api, cov, up, [n], u8)
            assert counts == [n // A] == _row_counts([n], A), tag
            law = synth.cov_law_reference(x, S, M, A, scale)
            worst = tc._check(tag, one, synth.cov_reference(x, S, M, A, scale), tc._bound(api, x, S, M, A, scale))
            print("cov grid %s: %d floats compared with the law, worst float64 error %.3f of its bound" % (tag, one.size, worst))
            assert one.shape == law.shape and np.array_equal(tc._bits(one), tc._bits(law)), (tag, _differing(one, law))
            cov.reset()
            cut, counts = _run(api, cov, up, cuts, u8)
            assert counts == _row_counts(cuts, A) and sum(counts) == n // A, (tag, counts)
            assert np.array_equal(tc._bits(cut), tc._bits(one)), (tag, "cut", _differing(cut, one))
        cov.close()


def test_the_cuts_are_what_the_docstring_says():
    """The closed form of the row counts at the three A: row ends only; a carried group into the direct store; mid-group
    and mid-row.  (No device work: the arithmetic of the grid above, stated once.)"""
    assert _row_counts([T, 2 * T, T, T], T) == [1, 2, 1, 1]
    assert _row_counts([T, 2 * T, T, 4 * T], 2 * T) == [0, 1, 1, 2]
    assert _row_counts([T, 2 * T, T, 13 * T], 5 * T) == [0, 0, 0, 3]
    assert [synth.cov_group(A)[1] for A in GRID_A] == [1, 2, 4]
