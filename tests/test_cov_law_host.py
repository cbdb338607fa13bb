"""The covariance estimator's summation order restated on the CPU (synth.fma32, synth.cov_law_reference), without a GPU:
what tests/test_gpu_cov_grid.py holds the device to bit for bit is itself held here to exact rational arithmetic.

  * fma32 against fractions.Fraction: a b + c formed exactly and rounded ONCE to float32 by integer arithmetic (_round32
    below; nothing of numpy's float conversions in it), on seeded random triples of four kinds, the tie that a rounding
    through float64 gets wrong, and the signed zeros;
  * cov_law_reference against the same law written a second time, entry by entry in Fractions (_law_entry): the folds
    of a restatement that groups from the right, takes another C or scales per group differ from it in their bits;
  * cov_law_reference against the float64 reference under test_gpu_cov's derived bound, against the exact integer Gram,
    and its symmetry in bits;
  * the class tables of tests/test_gpu_beam_grid.py and tests/test_gpu_cov_grid.py: every (KP, RT) of beam.h and every
    NT of cov.h, each at both edges of its range.  beam_kp, beam_rt and cov_nt are restated here from the headers."""
import struct
from fractions import Fraction

import numpy as np
import pytest

import test_gpu_beam_grid as bg
import test_gpu_cov as tc
import test_gpu_cov_grid as cg
from simplefe_amd import synth

T = 64


# ---------------------------------------------------------------------------------------- exact arithmetic
def _frac(v):
    return Fraction(float(v))                    # a float32 is a dyadic rational: exact


def _round32(q, zero_sign=0):
    """The float32 nearest to the Fraction q, ties to even, as its 32 bits; an exact zero takes zero_sign."""
    if q == 0:
        return 0x80000000 if zero_sign else 0
    sign, q = (0x80000000, -q) if q < 0 else (0, q)
    e = q.numerator.bit_length() - q.denominator.bit_length()       # 2^(e-1) < q < 2^(e+1)
    if Fraction(2) ** e > q:
        e -= 1                                                      # now 2^e <= q < 2^(e+1)
    e = max(e, -126)                                                # subnormals share the exponent of the smallest normal
    m = q / Fraction(2) ** (e - 23)                                 # the mantissa in units of the last place
    n = m.numerator // m.denominator
    rem = m - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n & 1):
        n += 1
    if n == 1 << 24:
        n, e = 1 << 23, e + 1
    if e > 127:
        return sign | 0x7f800000
    if n < 1 << 23:
        return sign | n                                             # subnormal (or zero by underflow)
    return sign | ((e + 127) << 23) | (n - (1 << 23))


def _bits32(v):
    return struct.unpack("<I", struct.pack("<f", float(v)))[0]


def _signbit(v):
    return _bits32(v) >> 31


def _fma_exact(a, b, c):
    """fmaf(a, b, c) of three finite float32 values as 32 bits: one rounding of the exact value (IEEE 754: an exact zero
    sum is +0 unless both terms are negative zeros or the product's and c's signs agree)."""
    q = _frac(a) * _frac(b) + _frac(c)
    sp = _signbit(a) ^ _signbit(b)
    if q == 0:
        if _frac(a) * _frac(b) == 0 and _frac(c) == 0:
            return _round32(q, sp & _signbit(c))
        return 0                                                    # x + (-x): +0 in round to nearest
    return _round32(q)


def _double_rounded(a, b, c):
    return np.float32(np.float64(a) * np.float64(b) + np.float64(c))


def _triples(n, seed):
    """n float32 triples of four kinds: free exponents, c near -a b (cancellation), c much larger than a b (the product
    decides a rounding of c's last place), and products built to land on or beside a tie of c's last place."""
    rng = np.random.default_rng(seed)
    k = n // 4
    f = lambda size, lo, hi: (rng.uniform(1.0, 2.0, size) * 2.0 ** rng.integers(lo, hi, size) * rng.choice([-1.0, 1.0], size)).astype(np.float32)
    a, b, c = f(n, -20, 20), f(n, -20, 20), f(n, -30, 30)
    c[k:2 * k] = (-(a[k:2 * k].astype(np.float64) * b[k:2 * k]) * (1.0 + rng.integers(-4, 5, k) * 2.0 ** -23)).astype(np.float32)
    c[2 * k:3 * k] = (np.abs(a[2 * k:3 * k].astype(np.float64) * b[2 * k:3 * k]) * 2.0 ** rng.integers(20, 27, k)).astype(np.float32)
    # a b = +-(half a unit of c's last place) (1 + d1 2^-23) (1 + d2 2^-23), d in -2 .. 2: exact ties, and with d1 = -d2
    # products a hair (2^-46) off a tie, which float64 cannot tell from it
    e = rng.integers(-10, 10, n - 3 * k)
    c[3 * k:] = (rng.uniform(1.0, 2.0, n - 3 * k).astype(np.float32).astype(np.float64) * 2.0 ** e).astype(np.float32)
    a[3 * k:] = (2.0 ** (e - 24.0) * rng.choice([-1.0, 1.0], n - 3 * k) * (1.0 + rng.integers(-2, 3, n - 3 * k) * 2.0 ** -23)).astype(np.float32)
    b[3 * k:] = (1.0 + rng.integers(-2, 3, n - 3 * k) * 2.0 ** -23).astype(np.float32)
    return a, b, c


def test_fma32_is_the_exact_sum_rounded_once():
    a, b, c = _triples(12000, 1)
    got = synth.fma32(a, b, c)
    assert got.dtype == np.float32 and got.shape == a.shape
    want = np.array([_fma_exact(*t) for t in zip(a, b, c)], np.uint32)
    bad = np.flatnonzero(got.view(np.uint32) != want)
    assert bad.size == 0, (bad.size, [(a[i], b[i], c[i]) for i in bad[:3]])
    # the set is hard enough to tell the double-rounded expression apart
    twice = _double_rounded(a, b, c)
    assert (twice.view(np.uint32) != want).sum() >= 10


TIE = (np.float32(2.0 ** -9 * (1 + 2.0 ** -23)), np.float32(2.0 ** -8 * (1 - 2.0 ** -23)), np.float32(128 + 2.0 ** -16))


@pytest.mark.parametrize("sa,sb", [(1, 1), (-1, 1), (1, -1), (-1, -1)])
def test_fma32_rounds_the_tie_once(sa, sb):
    """a b = 2^-17 (1 - 2^-46) sits just below half a unit of c's last place: the result is c.  float64 rounds the sum
    up to the tie, and the tie then goes to the even neighbour c + 2^-16."""
    a, b, c = sa * TIE[0], sb * TIE[1], sa * sb * TIE[2]
    assert float(c) == sa * sb * (128 + 2.0 ** -16)
    got = synth.fma32(a, b, c)
    assert _bits32(got) == _bits32(c) == _fma_exact(a, b, c)
    assert float(_double_rounded(a, b, c)) == sa * sb * (128 + 2.0 ** -15)      # the expression this is not


def test_fma32_signed_zeros_and_shapes():
    pz, nz = np.float32(0.0), np.float32(-0.0)
    a, b, _ = _triples(400, 2)
    for z in (pz, nz):                                              # a b + (+-0) is the rounded product
        got = synth.fma32(a, b, z)
        assert np.array_equal(got.view(np.uint32), np.array([_fma_exact(x, y, z) for x, y in zip(a, b)], np.uint32))
        assert np.array_equal(got, (a.astype(np.float64) * b).astype(np.float32))
    for x, y, z in [(pz, 3.0, pz), (pz, 3.0, nz), (nz, 3.0, pz), (nz, 3.0, nz), (pz, -3.0, nz), (nz, -3.0, nz), (2.0, 3.0, -6.0),
                    (-2.0, 3.0, 6.0)]:
        x, y, z = np.float32(x), np.float32(y), np.float32(z)
        assert _bits32(synth.fma32(x, y, z)) == _fma_exact(x, y, z), (x, y, z)
    assert _bits32(synth.fma32(nz, 3.0, nz)) == 0x80000000 and _bits32(synth.fma32(pz, 3.0, nz)) == 0
    # broadcasting, the smallest subnormal product, overflow, NaN
    assert synth.fma32(np.ones((3, 1), np.float32), np.ones((1, 4), np.float32), np.float32(1)).shape == (3, 4)
    tiny = np.float32(2.0 ** -75)
    assert _bits32(synth.fma32(tiny, tiny, pz)) == _fma_exact(tiny, tiny, pz) == 0         # 2^-150: a tie, to even
    assert _bits32(synth.fma32(tiny, np.float32(2.0 ** -74 * 1.5), pz)) == 2               # 1.5 2^-149: a tie, to even
    big = np.float32(2.0 ** 127)
    assert np.isposinf(synth.fma32(big, np.float32(2), big)) and np.isnan(synth.fma32(np.float32(np.nan), 1, 1))


# ---------------------------------------------------------------------------------------- the law, a second time
def _group(A):
    c = 1
    while c * c < A // T:
        c *= 2
    return c


def _f32(bits):
    return struct.unpack("<f", struct.pack("<I", bits))[0]


def _law_entry(u, v, A, scale):
    """One entry of one row by the header's words, in Fractions with _round32 after every operation: u, v the A float32
    values of the entry's two rows of U."""
    add = lambda p, q: _f32(_round32(_frac(p) + _frac(q)))
    C, AC = _group(A), A // T
    row = 0.0
    for g in range(0, AC, C):
        group = 0.0
        for ch in range(g, min(g + C, AC)):
            part = 0.0
            for m in range(ch * T, (ch + 1) * T):
                part = _f32(_fma_exact(u[m], v[m], part))
            group = add(group, part)
        row = add(row, group)
    return _round32(_frac(row) * _frac(np.float32(scale)))


@pytest.mark.parametrize("A", [T, 2 * T, 5 * T, 17 * T])
def test_law_reference_is_the_header_order_in_exact_arithmetic(A):
    """S = 2, M = 2, two rows: five entries of every row and band, among them a diagonal one and both of a mirrored pair.
    The scale is no power of two, so where it multiplies shows in the bits."""
    S, M, scale = 2, 2, 0.75 / A
    x = np.stack([synth.synth_cf32(M * 2 * A, ch=40 + s).view(np.complex64).reshape(M, 2 * A) for s in range(S)])
    law = synth.cov_law_reference(x, S, M, A, scale)
    assert law.shape == (M, 2, 2 * S, 2 * S) and law.dtype == np.float32
    assert (synth.cov_group(A)[1], A // T) in ((1, 1), (2, 2), (4, 5), (8, 17))
    U = synth.cov_columns(x, S, M).astype(np.float32)
    for k in range(M):
        for r in range(2):
            for i, j in ((0, 0), (0, 3), (3, 0), (1, 2), (2, 3)):
                want = _law_entry(U[k, i, r * A:(r + 1) * A], U[k, j, r * A:(r + 1) * A], A, scale)
                assert _bits32(law[k, r, i, j]) == want, (A, k, r, i, j)


@pytest.mark.parametrize("S", [1, 9, 17])
def test_law_reference_is_within_the_derived_bound_of_float64(S):
    from simplefe_amd import api
    M = 2
    for A in (64, 128, 320, 1088):
        t, c = api.cov_plan(S, M, A)
        assert (t, c) == synth.cov_group(A) == (T, _group(A))           # the library's plan, the header's formula
        n = 2 * A + T
        _, x = tc._input(S, M, tc.NMAX, False)
        x = np.ascontiguousarray(x[:, :, :n])
        law = synth.cov_law_reference(x, S, M, A, 1.0 / A)
        assert law.shape == (M, n // A, 2 * S, 2 * S) and n // A >= 2
        tc._check("law S=%d A=%d" % (S, A), law, synth.cov_reference(x, S, M, A, 1.0 / A), tc._bound(api, x, S, M, A, 1.0 / A))


@pytest.mark.parametrize("scale", [1.0, 0.5])
def test_law_reference_gives_the_exact_gram_of_small_integers(scale):
    S, M, A = 9, 2, 5 * T
    rng = np.random.default_rng(6)
    v = rng.integers(-8, 9, (S, M, 2 * A, 2))
    x = (v[..., 0] + 1j * v[..., 1]).astype(np.complex64)
    u = v.transpose(1, 0, 3, 2).reshape(M, 2 * S, 2, A).astype(np.int64)
    want = np.einsum("kira,kjra->krij", u, u)
    got = synth.cov_law_reference(x, S, M, A, scale)
    assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), scale * want.astype(np.float64))
    assert not np.array_equal(want[:, 0], want[:, 1]) and not np.array_equal(want, want.transpose(0, 1, 3, 2)[:, ::-1])


def test_law_reference_rows_are_symmetric_in_their_bits():
    S, M, A = 9, 2, 17 * T
    _, x = tc._input(S, M, tc.NMAX, True)
    law = synth.cov_law_reference(np.ascontiguousarray(x[:, :, :A]), S, M, A, 1.0 / A)
    assert np.array_equal(tc._bits(law), tc._bits(law.transpose(0, 1, 3, 2))) and np.abs(law).min() > 0


# ---------------------------------------------------------------------------------------- the class tables
def _beam_kp(S):            # beam.h: the smallest power of two with 4 kp >= S
    k = 1
    while 4 * k < S:
        k *= 2
    return k


def _beam_rt(B):            # beam.h: the smallest power of two with 8 rt >= B
    r = 1
    while 8 * r < B:
        r *= 2
    return r


def _cov_nt(S):             # cov.h
    return (2 * S + 15) // 16


def test_the_beam_grid_reaches_every_class_at_both_edges():
    classes = {(kp, rt) for kp in (1, 2, 4, 8, 16) for rt in (1, 2, 4, 8)}
    assert set(bg.CLASSES) == classes and len(classes) == 20
    for (kp, rt), shapes in bg.CLASSES.items():
        assert len(shapes) == 4 and {(_beam_kp(S), _beam_rt(B)) for S, B in shapes} == {(kp, rt)}
        s_lo, s_hi = min(S for S, _ in shapes), max(S for S, _ in shapes)
        b_lo, b_hi = min(B for _, B in shapes), max(B for _, B in shapes)
        assert set(shapes) == {(s_lo, b_lo), (s_lo, b_hi), (s_hi, b_lo), (s_hi, b_hi)}
        assert (s_lo == 1 or _beam_kp(s_lo - 1) < kp) and (s_hi == 64 or _beam_kp(s_hi + 1) > kp)
        assert (b_lo == 1 or _beam_rt(b_lo - 1) < rt) and (b_hi == 64 or _beam_rt(b_hi + 1) > rt)
    assert {(_beam_kp(S), _beam_rt(B)) for S, B in bg.STRIDE_SHAPES} == {(1, 1), (16, 1)}


def test_the_cov_grid_reaches_every_class_at_both_edges():
    assert {_cov_nt(S) for S in cg.GRID_S} == set(range(1, 9))
    for nt in range(1, 9):
        mine = [S for S in cg.GRID_S if _cov_nt(S) == nt]
        assert (min(mine) == 1 or _cov_nt(min(mine) - 1) == nt - 1) and (max(mine) == 64 or _cov_nt(max(mine) + 1) == nt + 1)
    assert cg.GRID_S == [1, 8, 9, 16, 17, 24, 25, 32, 33, 40, 41, 48, 49, 56, 57, 64]
    assert cg.GRID_A == (T, 2 * T, 5 * T) and cg.CUT_CHUNKS == [1, 2, 1]
