"""The Viterbi decoder (sfe_dsp_vit_*) without a GPU: the C ABI's declarations and exports, the encoder against a
restatement and a hand-written vector, the host plan -- the reference of the device's bits -- against an independent numpy
float32 restatement of the law written here, bit for bit, what the law corrects and recovers, every refusal of plan, create
and encode, the LDS bound's formula at its edges, and the build lists."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import vit_cases as vc
from simplefe_amd import synth
from vit_cases import encode_np, law_np, soft_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "sfe_dsp.h")
VIT_FUNCS = ("sfe_dsp_vit_encode", "sfe_dsp_vit_footprint", "sfe_dsp_vit_plan", "sfe_dsp_vit_create", "sfe_dsp_vit_process_stream",
             "sfe_dsp_vit_destroy")
F32 = np.float32
# (K, generators)
CODES = [(3, (7, 5)), (7, (0o171, 0o133)), (7, (0o133, 0o171, 0o165)), (8, (0o247, 0o371)), (9, (0o561, 0o753))]
CODE_IDS = ["K3", "K7", "K7n3", "K8", "K9"]
# rate-3/4 patterns of period 3: four of a period's positions are kept (n = 2: the usual one; n = 3: four of nine)
PUNCT = {2: [[1, 1], [1, 0], [0, 1]], 3: [[1, 1, 0], [1, 0, 0], [0, 0, 1]]}
LDS_BUDGET = 134400
NOISE_SEED = 3


@pytest.fixture(scope="module")
def L():
    from simplefe_amd import lib
    return lib.load()


@pytest.fixture(scope="module")
def api():
    from simplefe_amd import api as a
    return a


# ---- the ABI
def test_header_declares_vit_abi_and_library_exports_it(L):
    from simplefe_amd import lib
    declared = set(re.findall(r"\b(sfe_dsp_vit_[a-z0-9_]+)\s*\(", open(HDR).read()))
    assert declared == set(VIT_FUNCS)
    for name in VIT_FUNCS:
        assert hasattr(L, name), name
        assert name in lib.SIGNATURES, name


# ---- the encoder
def test_encoder_hand_written_vector(api):
    """K = 3, (7, 5), payload 1011 and two tail bits: the textbook's 11 10 00 01 01 11."""
    assert api.vit_encode(3, (7, 5), [1, 0, 1, 1]).tolist() == [1, 1, 1, 0, 0, 0, 0, 1, 0, 1, 1, 1]
    assert api.vit_encode(3, (7, 5), [1, 0, 1, 1], terminated=False).tolist() == [1, 1, 1, 0, 0, 0, 0, 1]
    # punctured by [[1, 1], [1, 0], [0, 1]]: positions (1, 1), (2, 0), (4, 1), (5, 0) are left out
    assert api.vit_encode(3, (7, 5), [1, 0, 1, 1], keep=PUNCT[2]).tolist() == [1, 1, 1, 0, 0, 1, 0, 1]


@pytest.mark.parametrize("code", CODES, ids=CODE_IDS)
@pytest.mark.parametrize("terminated", [True, False])
def test_encoder_against_the_restatement(api, code, terminated):
    K, gen = code
    for n_info in (1, 5, 64, 200):
        bits = synth.vit_bits(n_info, 100 + n_info)
        for keep in (None, PUNCT.get(len(gen))):
            want = encode_np(K, gen, bits, keep, terminated)[0]
            got = api.vit_encode(K, gen, bits, keep, terminated)
            assert np.array_equal(got, want), (n_info, keep)
            assert api.vit_plan(K, gen, n_info, keep, terminated) == want.size


# ---- the plan against the restatement, bit for bit
@pytest.mark.parametrize("code", CODES, ids=CODE_IDS)
@pytest.mark.parametrize("terminated", [True, False], ids=["terminated", "truncated"])
@pytest.mark.parametrize("n_info", [1, 5, 64, 200])
def test_plan_equals_the_numpy_restatement(api, code, terminated, n_info):
    K, gen = code
    for keep in (None, PUNCT.get(len(gen))):
        x = soft_inputs(K, gen, n_info, keep, terminated, 7 * K + n_info)
        by, rec, st = api.vit_plan(K, gen, n_info, keep, terminated, x=x)
        for b in range(x.shape[0]):
            wby, wm, wc, wst = law_np(K, gen, n_info, x[b], keep, terminated)
            assert np.array_equal(by[b], wby) and int(rec[b, 0]) == wm and int(rec[b, 1]) == wc and st[b] == wst, (keep, b)
        # all zeros: all-zero bits, metric +0, nothing disagrees
        assert not by[2].any() and rec[2].tolist() == [0, 0] and st[2] == 0


@pytest.mark.parametrize("code", vc.GRID_CODES, ids=vc.GRID_CODE_IDS)
def test_plan_and_encoder_equal_the_restatement_over_the_grid(api, code):
    """vit_cases' grid -- K = 3 .. 9 with 2, 3 and 4 generators, no puncturing and periods 3, 17 and 32 (the last two reach
    into the second word of the keep mask), both endings, n_info 1, 40 and 131 -- on noisy, integer-valued and all-zero
    rows: the plan is the numpy restatement bit for bit, the encoder is encode_np and n_soft is its length."""
    K, gen = code
    for name, keep, terminated, n_info, seed in vc.grid_cases(K, gen):
        bits = synth.vit_bits(n_info, seed)
        coded = encode_np(K, gen, bits, keep, terminated)[0]
        assert np.array_equal(api.vit_encode(K, gen, bits, keep, terminated), coded), (name, terminated, n_info)
        assert api.vit_plan(K, gen, n_info, keep, terminated) == coded.size
        x = soft_inputs(K, gen, n_info, keep, terminated, seed)
        by, rec, st = api.vit_plan(K, gen, n_info, keep, terminated, x=x)
        for b in range(x.shape[0]):
            wby, wm, wc, wst = law_np(K, gen, n_info, x[b], keep, terminated)
            assert np.array_equal(by[b], wby) and int(rec[b, 0]) == wm and int(rec[b, 1]) == wc and st[b] == wst, (name, terminated, n_info, b)
        assert not by[2].any() and rec[2].tolist() == [0, 0] and st[2] == 0


def test_plan_input_modes_status_in_and_failures(api):
    """BPSK and QPSK rows give the bits of SOFT rows on the extracted components; a NaN or an infinity anywhere among the
    n_soft values is status 1, one just outside them is not read; a nonzero status_in word is status 2."""
    from simplefe_amd import lib
    K, gen, n_info, skip = 7, (0o171, 0o133), 45, 3
    x = soft_inputs(K, gen, n_info, None, True, 5)[:2]
    want = api.vit_plan(K, gen, n_info, x=x)
    n_soft = x.shape[1]
    bp = np.full((2, skip + n_soft + 2), np.nan + 0j, np.complex64)
    bp[:, skip:skip + n_soft].real = x
    bp[:, skip:skip + n_soft].imag = np.inf                                         # the imaginary parts are not read
    got = api.vit_plan(K, gen, n_info, in_mode=lib.VIT_IN_BPSK, skip=skip, x=bp)
    assert all(np.array_equal(u, v) for u, v in zip(got, want))
    qp = np.full((2, skip + n_soft // 2 + 1), np.nan + 0j, np.complex64)
    qp[:, skip:skip + n_soft // 2] = x[:, 0::2] + 1j * x[:, 1::2]
    got = api.vit_plan(K, gen, n_info, in_mode=lib.VIT_IN_QPSK, skip=skip, x=qp)
    assert all(np.array_equal(u, v) for u, v in zip(got, want))
    for at in (0, 17, n_soft - 1):
        for bad in (np.nan, np.inf, -np.inf):
            xb = np.concatenate([x, np.zeros((2, 1), F32)], axis=1)
            xb[1, at] = bad
            xb[0, n_soft] = bad                                                     # beyond burst 0's values
            by, rec, st = api.vit_plan(K, gen, n_info, x=xb)
            assert st.tolist() == [0, 1] and not by[1].any() and rec[1].tolist() == [0x7fc00000, 0]
            assert np.array_equal(by[0], want[0][0]) and np.array_equal(rec[0], want[1][0])
    by, rec, st = api.vit_plan(K, gen, n_info, x=x, status_in=[0, 3])
    assert st.tolist() == [0, 2] and not by[1].any() and rec[1].tolist() == [0x7fc00000, 0] and np.array_equal(by[0], want[0][0])


# ---- what the law corrects and recovers
def test_four_flipped_positions_are_corrected(api):
    """K = 7 (0o171, 0o133), free distance 10: any four flipped positions of a terminated 40-bit burst of +-1 decode to the
    payload.  300 random patterns."""
    K, gen, n_info = 7, (0o171, 0o133), 40
    rng = np.random.default_rng(11)
    rows, want = [], []
    for i in range(300):
        bits = rng.integers(0, 2, n_info).astype(np.uint8)
        r = synth.vit_soft(api.vit_encode(K, gen, bits))
        r[rng.choice(r.size, 4, replace=False)] *= -1
        rows.append(r)
        want.append(np.packbits(bits))
    by, rec, st = api.vit_plan(K, gen, n_info, x=np.stack(rows))
    assert not st.any() and np.array_equal(by, np.stack(want))
    assert (rec[:, 1] == 4).all() and (rec[:, 0].copy().view(F32) == 92 - 8).all()


@pytest.mark.parametrize("code", CODES[:4], ids=CODE_IDS[:4])
def test_recovery_under_noise(api, code):
    """200 payload bits of BPSK at Eb/N0 = 3 dB: the raw hard decisions hold errors, the decoded payload none.  The seed is
    the first of 1 .. 12 at which all four codes decode clean: K = 3, of free distance 5, leaves one wrong bit at seeds 1,
    2, 5 and 6 (a property of that code at 3 dB, measured on the CPU), the other three codes none at any of the twelve.
    Seed 3 gives 28, 34, 77 and 31 raw errors."""
    K, gen = code
    bits = synth.vit_bits(200, NOISE_SEED)
    coded = api.vit_encode(K, gen, bits)
    r = synth.vit_soft(coded, 3.0, 1.0 / len(gen), seed=NOISE_SEED)
    raw = int(((r < 0) != (coded == 1)).sum())
    by, rec, st = api.vit_plan(K, gen, 200, x=r)
    wrong = int(np.unpackbits(by[0] ^ np.packbits(bits)).sum())
    print("K = %d, n = %d: %d raw errors among %d positions, %d decoded, count %d" % (K, len(gen), raw, coded.size, wrong, rec[0, 1]))
    assert st[0] == 0 and raw > 0 and wrong == 0 and rec[0, 1] == raw


# ---- refusals
GOOD = dict(K=7, n_gen=2, gen=(0o171, 0o133), keep=None, P=1, terminated=1, n_info=64, in_mode=0, skip=0)
BAD = {"K = 2": dict(K=2, gen=(3, 1)), "K = 10": dict(K=10), "n_gen = 1": dict(n_gen=1), "n_gen = 5": dict(n_gen=5, gen=(1, 2, 3, 4, 5)),
       "a zero generator": dict(gen=(0o171, 0)), "a generator of K + 1 bits": dict(gen=(0o171, 0o200)), "null generators": dict(gen=None),
       "terminated = 2": dict(terminated=2), "terminated = -1": dict(terminated=-1), "n_info = 0": dict(n_info=0), "n_info = -1": dict(n_info=-1),
       "n_info = 8193": dict(n_info=8193), "P = 0": dict(keep=[[1, 1]], P=0), "P = 33": dict(keep=[[1, 1]] * 33, P=33),
       "keep = 2": dict(keep=[[1, 2]], P=1), "nothing kept": dict(keep=[[0, 0], [0, 0]], P=2),
       "nothing kept within T": dict(keep=[[0, 0]] * 31 + [[1, 1]], P=32, n_info=3)}
BAD_MODE = {"in_mode = 3": dict(in_mode=3), "in_mode = -1": dict(in_mode=-1), "skip = -1": dict(in_mode=1, skip=-1),
            "skip with SOFT": dict(skip=1), "skip = 2^24 + 1": dict(in_mode=2, skip=(1 << 24) + 1),
            "K = 9 beyond the LDS bound": dict(K=9, gen=(0o561, 0o753), n_info=4176)}


def _args(kw):
    a = dict(GOOD, **kw)
    gen = None if a["gen"] is None else (C.c_uint32 * len(a["gen"]))(*a["gen"])
    keep = None if a["keep"] is None else (C.c_uint8 * (len(a["keep"]) * len(a["keep"][0])))(*[v for row in a["keep"] for v in row])
    return a, gen, keep


def _plan_rc(L, **kw):
    a, gen, keep = _args(kw)
    return L.sfe_dsp_vit_plan(a["K"], a["n_gen"], gen, keep, a["P"], a["terminated"], a["n_info"], a["in_mode"], a["skip"], None, 0, None, 0, None, 0,
                              None, None, None)


def _create_rc(L, **kw):
    a, gen, keep = _args(kw)
    h = C.c_void_p()
    rc = L.sfe_dsp_vit_create(a["K"], a["n_gen"], gen, keep, a["P"], a["terminated"], a["n_info"], a["in_mode"], a["skip"], 0, C.byref(h))
    return rc, h.value


def _encode_rc(L, **kw):
    a, gen, keep = _args(kw)
    n = max(a["n_info"], 0)
    bits, k = (C.c_uint8 * max(n, 1))(), C.c_size_t(7)
    rc = L.sfe_dsp_vit_encode(a["K"], a["n_gen"], gen, keep, a["P"], a["terminated"], bits, n, None, C.byref(k))
    return rc, k.value


@pytest.mark.parametrize("why", list(BAD) + list(BAD_MODE))
def test_plan_create_and_encode_refuse_with_a_message(L, why):
    """Create refuses before it looks for a device; encode checks the code alone."""
    from simplefe_amd import lib
    kw = BAD.get(why) or BAD_MODE[why]
    assert _plan_rc(L, **kw) == lib.SFE_EINVAL
    assert L.sfe_dsp_last_error().startswith(b"vit: "), L.sfe_dsp_last_error()
    rc, h = _create_rc(L, **kw)
    assert rc == lib.SFE_EINVAL and not h and L.sfe_dsp_last_error().startswith(b"vit: ")
    if why in BAD:
        assert _encode_rc(L, **kw) == (lib.SFE_EINVAL, 0) and L.sfe_dsp_last_error().startswith(b"vit: ")


def test_the_limits_themselves_are_accepted_and_other_refusals(L, api):
    from simplefe_amd import lib
    assert _plan_rc(L) == lib.SFE_OK
    assert _plan_rc(L, K=3, gen=(7, 1), n_info=1, terminated=0) == lib.SFE_OK
    assert _plan_rc(L, K=9, n_gen=4, gen=(511, 1, 256, 0o753), n_info=4092, keep=[[0, 0, 0, 1]] + [[0, 0, 0, 0]] * 31, P=32) == lib.SFE_OK
    assert _plan_rc(L, n_info=8192, in_mode=2, skip=1 << 24) == lib.SFE_OK
    assert _encode_rc(L) == (lib.SFE_OK, 2 * 70)
    gen = (C.c_uint32 * 2)(0o171, 0o133)
    bits, coded, k = (C.c_uint8 * 8)(0, 1, 2, 0, 0, 0, 0, 0), (C.c_uint8 * 64)(), C.c_size_t(0)
    assert L.sfe_dsp_vit_encode(7, 2, gen, None, 1, 1, bits, 8, coded, C.byref(k)) == lib.SFE_EINVAL         # a bit that is 2
    assert L.sfe_dsp_last_error().startswith(b"vit: ")
    assert L.sfe_dsp_vit_encode(7, 2, gen, None, 1, 1, None, 8, coded, C.byref(k)) == lib.SFE_EINVAL
    assert L.sfe_dsp_vit_encode(7, 2, gen, None, 1, 1, bits, 8, coded, None) == lib.SFE_EINVAL
    # soft values to decode need somewhere to put the bytes, and rows as long as the burst
    x = np.zeros((2, 2 * 70), F32)
    fp, by = x.ctypes.data_as(C.POINTER(C.c_float)), (C.c_uint8 * 16)()
    assert L.sfe_dsp_vit_plan(7, 2, gen, None, 1, 1, 64, 0, 0, fp, 140, None, 2, None, 8, None, None, None) == lib.SFE_EINVAL
    assert L.sfe_dsp_last_error().startswith(b"vit: ")
    assert L.sfe_dsp_vit_plan(7, 2, gen, None, 1, 1, 64, 0, 0, fp, 139, None, 2, by, 8, None, None, None) == lib.SFE_ERANGE
    assert L.sfe_dsp_vit_plan(7, 2, gen, None, 1, 1, 64, 0, 0, fp, 140, None, 2, by, 7, None, None, None) == lib.SFE_ERANGE
    assert L.sfe_dsp_vit_plan(7, 2, gen, None, 1, 1, 64, 0, 0, fp, 140, None, 1 << 31, by, 8, None, None, None) == lib.SFE_EINVAL
    assert L.sfe_dsp_vit_plan(7, 2, gen, None, 1, 1, 64, 0, 0, fp, 140, None, 2, by, 8, None, None, None) == lib.SFE_OK
    with pytest.raises(ValueError):
        api.vit_plan(7, (0o171, 0o133), 64, keep=[[1, 1, 1]])


def test_create_without_a_gpu_is_enodev(L):
    from simplefe_amd import lib
    rc, h = _create_rc(L)
    if h:
        assert L.sfe_dsp_vit_destroy(h) == lib.SFE_OK
    assert rc == (lib.SFE_OK if os.path.exists("/dev/kfd") else lib.SFE_ENODEV)


# ---- the LDS bound
def footprint(K, n, n_info, terminated=True):
    """vit.h's constexprs, restated: (survivors + packed bits, staged, bursts per workgroup)."""
    T = n_info + (K - 1 if terminated else 0)
    base = T * max(1 << (K - 1), 64) // 8 + ((n_info + 7) // 8 + 7) // 8 * 8
    soft = (T * n * 4 + 7) // 8 * 8
    staged = base + soft <= LDS_BUDGET
    return base, staged, 0 if base > LDS_BUDGET else max(1, min(4, LDS_BUDGET // (base + (soft if staged else 0))))


def test_the_lds_bound_at_its_edges(L, api):
    from simplefe_amd import lib
    for K, n, n_info, term in [(3, 2, 1, True), (7, 2, 256, True), (7, 2, 8192, True), (7, 3, 8192, True), (7, 4, 8192, False), (8, 2, 8192, True),
                               (9, 2, 2048, True), (9, 2, 4175, True), (9, 2, 4176, True), (9, 4, 4183, False), (9, 4, 4184, False), (9, 2, 8192, True),
                               (7, 2, 8191, True), (6, 3, 6700, True), (6, 3, 6701, True), (4, 2, 1390, True), (4, 2, 2790, False)]:
        assert api.vit_footprint(K, n, n_info, term) == footprint(K, n, n_info, term), (K, n, n_info, term)
    # K = 9: the last T whose survivors and bits fit, and the first that does not
    assert footprint(9, 2, 4175)[2] == 1 and footprint(9, 2, 4176)[2] == 0 and footprint(9, 2, 4183, False)[2] == 1 and footprint(9, 2, 4184, False)[2] == 0
    gen = dict(K=9, gen=(0o561, 0o753))
    assert _plan_rc(L, n_info=4175, **gen) == lib.SFE_OK and _plan_rc(L, n_info=4176, **gen) == lib.SFE_EINVAL
    assert b"exceed the 134400 bytes" in L.sfe_dsp_last_error() and b"T * max(2^(K-1), 64) / 8" in L.sfe_dsp_last_error()
    assert _plan_rc(L, n_info=4183, terminated=0, **gen) == lib.SFE_OK and _plan_rc(L, n_info=4184, terminated=0, **gen) == lib.SFE_EINVAL
    # every K <= 8 fits at the longest burst; K = 7, n = 2 stages its soft values there, n = 3 does not
    assert all(footprint(K, 2, 8192)[2] >= 1 for K in range(3, 9))
    assert footprint(7, 2, 8192)[1] and not footprint(7, 3, 8192)[1]


def test_build_lists_name_the_vit_files():
    from simplefe_amd import build
    assert "api_vit.hip" in build.HOST_SOURCES and "vit.hip" in build.EXACT_SOURCES and build.SCRATCH_FREE["vit.hip"]
    assert build.KERNEL_FILES["vit"][:2] == ("vit.hip", "vit.h")
    assert "vit.hip" in open(os.path.join(ROOT, "CMakeLists.txt")).read()
