"""Every class of the Viterbi kernel on the GPU -- vit_kernel<n_gen 2 .. 4, states per lane 1 / 2 / 4> -- over vit_cases'
grid: K = 3 .. 9 (idle lanes below K = 7), patterns of period 3, 17 and 32 (the last two use the second word of the keep
mask), both endings, sizes that leave a partial last period.  The grid is held to the numpy restatement of the law and
to the plan, bit for bit, through guarded buffers; each class is launched with its soft values staged in LDS and read
from global memory; footprints of 2 and 3 bursts per workgroup; BPSK and QPSK rows at a four-generator code."""
import numpy as np
import pytest

import vit_cases as vc
from vit_cases import rows_of, run, same

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def api():
    from simplefe_amd import api as a
    return a


@pytest.fixture(scope="module")
def L():
    from simplefe_amd import lib
    return lib


@pytest.mark.parametrize("code", vc.GRID_CODES, ids=vc.GRID_CODE_IDS)
def test_the_grid_equals_the_restatement_and_the_plan(api, code):
    """Per code 4 patterns x 2 endings x 3 sizes, five bursts a call -- noisy, integer-valued, zeros, two more noisy:
    bytes, both record words and status equal law_np's and the plan's."""
    K, gen = code
    for name, keep, terminated, n_info, seed in vc.grid_cases(K, gen):
        x = rows_of(api, K, gen, n_info, keep, terminated, 5, seed)
        want = api.vit_plan(K, gen, n_info, keep, terminated, x=x)
        h = api.Vit(K, gen, n_info, keep, terminated)
        got = run(api, h, x, in_pad=n_info % 3, out_pad=1 + n_info % 2, lead=1 + n_info % 4)
        h.close()
        why = (name, terminated, n_info)
        assert api.vit_footprint(K, len(gen), n_info, terminated)[1:] == (True, 4), why
        assert not want[2].any() and not want[0][2].any() and want[1][2].tolist() == [0, 0], why
        assert same(got, want), why
        for b in range(5):
            wby, wm, wc, wst = vc.law_np(K, gen, n_info, x[b], keep, terminated)
            assert np.array_equal(got[0][b], wby) and got[1][b].tolist() == [wm, wc] and got[2][b] == wst, why + (b,)


def first_unstaged(api, K, n, terminated):
    """The smallest n_info whose soft values no longer fit in LDS beside the survivors, or None where every n_info fits."""
    lo, hi = 1, 8192
    if api.vit_footprint(K, n, hi, terminated)[1]:
        return None
    while lo < hi:
        mid = (lo + hi) // 2
        if api.vit_footprint(K, n, mid, terminated)[1]:
            lo = mid + 1
        else:
            hi = mid
    return lo


# (n_gen, states per lane) -> K: one code per kernel class
CLASS_K = {1: 7, 2: 8, 4: 9}
CLASSES = [(n, spl) for n in (2, 3, 4) for spl in (1, 2, 4)]


@pytest.mark.parametrize("staged", [True, False], ids=["staged", "unstaged"])
@pytest.mark.parametrize("cls", CLASSES, ids=["n%d-spl%d" % c for c in CLASSES])
def test_every_class_staged_and_unstaged(api, cls, staged):
    """The period-32 pattern, three bursts, truncated (the end state is searched for): staged at n_info = 131, and at the
    first n_info at which vit_footprint reports the soft values left in global memory -- some thousand steps.  Against the
    plan, which tests/test_vit_host.py holds to the restatement.  One class has no unstaged launch: with two generators
    and one state per lane (K <= 7) the longest burst, 8192 + 6 steps of 16 bytes and 1024 bytes of bits, fits the LDS
    budget, which is asserted here in its place."""
    n, spl = cls
    K = CLASS_K[spl]
    gen, keep = vc.GENS[K][:n], vc.LONG[32, n]
    n_info = 131 if staged else first_unstaged(api, K, n, False)
    if n_info is None:
        assert cls == (2, 1) and all(api.vit_footprint(k, 2, 8192, True)[1] for k in range(3, 8))
        return
    base, is_staged, waves = api.vit_footprint(K, n, n_info, False)
    assert is_staged == staged and waves >= 1 and (staged or api.vit_footprint(K, n, n_info - 1, False)[1])
    x = rows_of(api, K, gen, n_info, keep, False, 3, 300 + 10 * K + n)
    want = api.vit_plan(K, gen, n_info, keep, False, x=x)
    h = api.Vit(K, gen, n_info, keep, False)
    got = run(api, h, x, in_pad=1, out_pad=3, lead=2)
    h.close()
    print("K = %d, n = %d, n_info = %d: %d bytes of survivors and bits, staged %s, %d bursts per workgroup" % (K, n, n_info, base, is_staged, waves))
    assert not want[2].any() and same(got, want)


# (K, n_gen, n_info, pattern period, bursts per workgroup): survivors, bits and staged soft values of 53 304 and 38 776 bytes
PER_GROUP = [(9, 3, 1200, 32, 2), (8, 4, 1200, 17, 3)]


@pytest.mark.parametrize("shape", PER_GROUP, ids=["two", "three"])
def test_two_and_three_bursts_per_workgroup(api, shape):
    """Five bursts, no multiple of either: the last workgroup has idle waves, and a wave's LDS starts at offsets no other
    test uses.  Against the plan, and every burst against a one-burst call at another address, bit for bit."""
    K, n, n_info, P, waves = shape
    gen, keep = vc.GENS[K][:n], vc.LONG[P, n]
    assert api.vit_footprint(K, n, n_info, True)[1:] == (True, waves)
    x = rows_of(api, K, gen, n_info, keep, True, 5, 40 + K)
    want = api.vit_plan(K, gen, n_info, keep, True, x=x)
    h = api.Vit(K, gen, n_info, keep, True)
    got = run(api, h, x, in_pad=3, out_pad=1, lead=2)
    assert not want[2].any() and same(got, want)
    for i in range(5):
        one = run(api, h, x[i:i + 1], in_pad=i % 4, out_pad=i % 5, lead=1 + i % 3)
        assert same(one, [v[i:i + 1] for v in got]), i
    h.close()


@pytest.mark.parametrize("terminated", [True, False], ids=["terminated", "truncated"])
def test_symbol_input_with_a_long_pattern(api, L, terminated):
    """K = 6 with four generators and the period-32 pattern: BPSK and QPSK rows -- what is not read is NaN or infinite --
    against SOFT rows of the extracted components, themselves the plan's.  An odd n_soft leaves the last QPSK symbol's
    imaginary part unread."""
    K, n_info, skip = 6, 45 if terminated else 44, 3
    gen, keep = vc.GENS[K], vc.LONG[32, 4]
    x = rows_of(api, K, gen, n_info, keep, terminated, 5, 9)
    n_soft = x.shape[1]
    h = api.Vit(K, gen, n_info, keep, terminated)
    want = run(api, h, x)
    h.close()
    assert not want[2].any() and same(want, api.vit_plan(K, gen, n_info, keep, terminated, x=x))
    bp = np.full((5, skip + n_soft + 2), np.nan + 0j, np.complex64)
    bp[:, skip:skip + n_soft].real = x
    bp[:, skip:skip + n_soft].imag = np.inf
    h = api.Vit(K, gen, n_info, keep, terminated, in_mode=L.VIT_IN_BPSK, skip=skip)
    assert same(run(api, h, bp, in_pad=1, lead=1), want)
    h.close()
    half = (n_soft + 1) // 2
    comp = np.full((5, 2 * half), np.nan, F32)
    comp[:, :n_soft] = x
    qp = np.full((5, skip + half + 1), np.nan + 0j, np.complex64)
    qp[:, skip:skip + half] = comp.view(np.complex64)
    h = api.Vit(K, gen, n_info, keep, terminated, in_mode=L.VIT_IN_QPSK, skip=skip)
    assert same(run(api, h, qp, in_pad=2, lead=3), want)
    h.close()
    print("n_soft = %d (%s)" % (n_soft, "odd" if n_soft & 1 else "even"))
